// Host execution of the engine's entry points for TINY calls ("a CPU backend implementing the same
// header"; BASELINE configs[0]: "DLEQ proof ... single prove + verify on CPU (plumbing, no GPU)").
//
// A single DLEQ verification through the GPU is a chain of ~10 kernel launches, ~1 ms whatever the size; the reference needs ~0.1 ms
// on one core (benches/dleq.rs:49-90).  For calls below a handful of terms the host toolbox therefore runs the group arithmetic HERE:
// the very header the kernels' point arithmetic is compiled from -- ge25519.h (extended coordinates, ristretto255 codec) -- compiled for
// the host by g++ over a field of 5 x 51-bit limbs with the same interface as the device's 9 x 29-bit one (host/fe51.h: a 64-bit core
// needs 25 products per multiplication instead of 98) -- behind the same zkp_toolbox.h calls, and also when no GPU context is given at all
// (ctx == NULL).  Same bytes as the device path (outputs are canonical encodings), checked by tests/test_host_backend.py against the
// oracle and by tests/test_gpu_toolbox.py against the GPU route.  This is product code: nothing under oracle/ is involved.
//
// Algorithms (host/host_backend.hpp has the interface):
//   msm_many      per MSM a Straus walk over signed radix-16 digits, table {1..8} P per distinct point of the MSM.  flags = ZKP_CT: the
//                 table entry is picked with masks over all eight entries and zero digits are added like any other (what
//                 curve25519-dalek's constant-time multiscalar_mul does, prover.rs:94); ZKP_VARTIME: indexed, zeros skipped.
//   msm_segments_n  zkp_msm_segments (11): msm_many's results with the TERM axis cut over the threads.  A thread walks the terms of its stretch segment by
//                 segment (the same Straus walk); a segment longer than a stretch leaves one partial sum per stretch, added at the end.
//   msm_optional  the same walk over n points with decode-or-None (verifier.rs:162-166, batch_verifier.rs:219-228).
//   decode_check  ristretto decode.
//   from_uniform_bytes  RFC 9496 section 4.3.4 (ristretto_from_uniform_bytes of ge25519.h: selects only, constant time), then the encoder.
//   hash_from_bytes_sha512  sha512_range of sha512.h (the kernel's SHA-512, byte loads on the host), then from_uniform_bytes.
//   mul_base_n / mul_points_n  zkp_mul_base / zkp_mul_points (8): the Straus walk above with one operand -- signed radix-16 digits over the
//                 table {1..8} P, 256 doublings + 65 additions; ZKP_CT keeps the masked look-ups and skips no digit (mul_base_n always).
//   add_points_n / sum_points_n  zkp_add_points / zkp_sum_points (9): decode, the complete addition of ge25519.h (a sign is a conditional negation of
//                 the cached operand), encode.  A sum is one serial chain here; the toolbox cuts long ones (sum_points_partial / _finish).
//   sc_scan_n / point_scan_n  zkp_sc_scan / zkp_scan_points (13): the term axis cut over the threads; a stretch is scanned from the identity, the
//                 stretch totals serially, and the rows before a stretch's first segment start take their carry in a second pass.
//   dlog_halve / dlog_base_range / dlog_base_n  zkp_dlog_base (10): baby-step / giant-step of dlog.h -- the point halved once, candidates walked by subtracting
//                 (m / 2) B, encode(2 H) of DLOG_GROUP consecutive candidates from one inversion (the serial form of Montgomery's trick), the probe of
//                 dlog.h.  The baby table is built here the same way and kept per (base, baby_bits) for the process behind a mutex; the dlog_point_*
//                 forms take the base and a signed flag (zkp_dlog_point), the others are those with B.
//   sc_*          the scalar kernels' bodies: sc25519.h (sc_invert, sc_from_wide, sc_mont) compiled for the host, element by element.
#include "host_backend.hpp"

#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#define ZKP_HOST_FE51 1        // this translation unit (and no other of the library) gets the 5 x 51-bit field under the device's point formulas
#include "../ge25519.h"
#include "../sha512.h"
#include "../sc25519.h"
#include "../dlog.h"

namespace zkp {
namespace hostbk {

namespace {

inline uint32_t decode(ge_p3& p, const uint8_t* enc) {
  uint32_t w[8];
  std::memcpy(w, enc, 32);
  return ristretto_decode(p, w);
}
inline void encode(uint8_t* out, const ge_p3& p) {
  uint32_t w[8];
  ristretto_encode(w, p);
  std::memcpy(out, w, 32);
}

// signed radix-16 digits of any 256-bit integer: s = sum d[i] 16^i, d[i] in [-8, 8) for i < 64, d[64] in {0, 1}
inline void recode16(int8_t d[65], const uint8_t s[32]) {
  int carry = 0;
  for (int i = 0; i < 64; ++i) {
    int v = ((s[i >> 1] >> (4 * (i & 1))) & 15) + carry;
    carry = v >= 8;
    d[i] = (int8_t)(v - 16 * carry);
  }
  d[64] = (int8_t)carry;
}

struct Table { ge_cached e[8]; };          // 1P .. 8P
inline void build_table(Table& t, const ge_p3& p) {
  ge_p3 acc = p;
  ge_to_cached(t.e[0], p);
  for (int k = 1; k < 8; ++k) {
    ge_add_cached(acc, acc, t.e[0]);
    ge_to_cached(t.e[k], acc);
  }
}
// acc += d * P with the table of P.  ct: every entry is touched, the sign is applied with a mask, d == 0 adds the neutral element
template <bool CT>
inline void add_digit(ge_p3& acc, const Table& t, int d) {
  if (!CT) {
    if (d == 0) return;
    if (d > 0) ge_add_cached(acc, acc, t.e[d - 1]);
    else ge_sub_cached(acc, acc, t.e[-d - 1]);
    return;
  }
  const uint32_t neg = (uint32_t)(d >> 7) & 1u;                   // d is an int8 value
  const uint32_t mag = (uint32_t)((d ^ -(int)neg) + (int)neg);      // |d| without a branch
  ge_cached sel;
  ge_cached_identity(sel);
  for (uint32_t k = 1; k <= 8; ++k) {
    const uint32_t x = mag ^ k;
    ge_cached_cmov(sel, t.e[k - 1], ((x - 1u) >> 31) & 1u);          // x == 0
  }
  ge_cached_cneg(sel, neg);
  ge_add_cached(acc, acc, sel);
}

template <bool CT>
void straus(ge_p3& acc, size_t k, const int8_t (*digits)[65], const Table* const* tables) {
  ge_identity(acc);
  for (int w = 64; w >= 0; --w) {
    if (w != 64) { ge_double<false>(acc, acc); ge_double<false>(acc, acc); ge_double<false>(acc, acc); ge_double<true>(acc, acc); }
    for (size_t i = 0; i < k; ++i) add_digit<CT>(acc, *tables[i], digits[i][w]);
  }
}

}  // namespace

int msm_many(uint32_t n_msm, const uint32_t* off, const uint8_t* scalars, const uint32_t* pidx, const uint8_t* points, uint32_t n_points, int flags,
             uint8_t* out, uint8_t* status) {
  if (n_msm == 0) return ZKP_OK;
  if (!off || !out || !status || off[0] != 0) return ZKP_ERR_ARG;
  const uint32_t T = off[n_msm];
  if (T && (!scalars || !pidx || !points)) return ZKP_ERR_ARG;
  // decode and tabulate each referenced point once
  std::vector<int32_t> slot(n_points, -1);
  std::vector<Table> tabs;
  std::vector<uint8_t> ok;
  for (uint32_t t = 0; t < T; ++t) {
    if (pidx[t] >= n_points) return ZKP_ERR_ARG;
    if (slot[pidx[t]] >= 0) continue;
    ge_p3 p;
    const uint32_t good = decode(p, points + 32 * (size_t)pidx[t]);
    slot[pidx[t]] = (int32_t)tabs.size();
    tabs.emplace_back();
    ok.push_back((uint8_t)good);
    if (good) build_table(tabs.back(), p);
  }
  std::vector<int8_t> dig;
  std::vector<const Table*> tp;
  for (uint32_t i = 0; i < n_msm; ++i) {
    if (off[i + 1] < off[i]) return ZKP_ERR_ARG;
    const size_t k = off[i + 1] - off[i];
    dig.resize(65 * (k ? k : 1));
    tp.resize(k);
    bool bad = false;
    for (size_t j = 0; j < k; ++j) {
      const uint32_t t = off[i] + (uint32_t)j;
      recode16(reinterpret_cast<int8_t(*)[65]>(dig.data())[j], scalars + 32 * (size_t)t);
      tp[j] = &tabs[slot[pidx[t]]];
      bad |= !ok[slot[pidx[t]]];
    }
    status[i] = bad ? 1 : 0;
    if (bad) { std::memset(out + 32 * (size_t)i, 0, 32); continue; }
    ge_p3 acc;
    if (flags == ZKP_CT) straus<true>(acc, k, reinterpret_cast<const int8_t(*)[65]>(dig.data()), tp.data());
    else straus<false>(acc, k, reinterpret_cast<const int8_t(*)[65]>(dig.data()), tp.data());
    encode(out + 32 * (size_t)i, acc);
  }
  return ZKP_OK;
}

// ---- multiscalar sums with long segments (zkp_mi355x.h (11)) ----
namespace {
// One thread's stretch [lo, hi) of the term axis: a table per distinct point the stretch uses, and per segment it meets one Straus walk over the
// terms the two share.  A segment that lies wholly inside is finished here (out, status); the others leave a partial sum for the caller.
struct SegPartial { uint32_t seg; bool bad; ge_p3 sum; };
void msm_stretch(uint32_t lo, uint32_t hi, uint32_t n_msm, const uint32_t* off, const uint8_t* scalars, const uint32_t* pidx, const uint8_t* points,
                 uint32_t n_points, int flags, uint8_t* out, uint8_t* status, std::vector<SegPartial>& partials) {
  std::map<uint32_t, uint32_t> slot;                 // point -> table (a stretch touches few of a large catalogue's points)
  std::vector<Table> tabs;
  std::vector<uint8_t> ok;
  std::vector<uint32_t> term_slot(hi - lo);
  for (uint32_t t = lo; t < hi; ++t) {
    const uint32_t pi = pidx ? pidx[t] : t;
    auto it = slot.find(pi);
    if (it == slot.end()) {
      ge_p3 p;
      const uint32_t good = decode(p, points + 32 * (size_t)pi);
      it = slot.emplace(pi, (uint32_t)tabs.size()).first;
      tabs.emplace_back();
      ok.push_back((uint8_t)good);
      if (good) build_table(tabs.back(), p);
    }
    term_slot[t - lo] = it->second;
  }
  std::vector<int8_t> dig;
  std::vector<const Table*> tp;
  uint32_t s = (uint32_t)(std::upper_bound(off, off + n_msm + 1, lo) - off) - 1;      // the segment of term lo
  for (; s < n_msm && off[s] < hi; ++s) {
    const uint32_t a = std::max(off[s], lo), b = std::min(off[s + 1], hi);
    if (a >= b) continue;                                                                // an empty segment inside the stretch
    const size_t k = b - a;
    dig.resize(65 * k);
    tp.resize(k);
    bool bad = false;
    for (size_t j = 0; j < k; ++j) {
      recode16(reinterpret_cast<int8_t(*)[65]>(dig.data())[j], scalars + 32 * (size_t)(a + j));
      tp[j] = &tabs[term_slot[a + j - lo]];
      bad |= !ok[term_slot[a + j - lo]];
    }
    ge_p3 acc;
    ge_identity(acc);
    if (!bad) {
      if (flags == ZKP_CT) straus<true>(acc, k, reinterpret_cast<const int8_t(*)[65]>(dig.data()), tp.data());
      else straus<false>(acc, k, reinterpret_cast<const int8_t(*)[65]>(dig.data()), tp.data());
    }
    if (a == off[s] && b == off[s + 1]) {
      status[s] = bad ? 1 : 0;
      if (bad) std::memset(out + 32 * (size_t)s, 0, 32);
      else encode(out + 32 * (size_t)s, acc);
    } else {
      partials.push_back({s, bad, acc});
    }
  }
}
}  // namespace

int msm_segments_n(uint32_t n_msm, const uint32_t* off, const uint8_t* scalars, const uint32_t* pidx, const uint8_t* points, uint32_t n_points, int flags,
                   int n_threads, uint8_t* out, uint8_t* status) {
  if (flags != ZKP_CT && flags != ZKP_VARTIME) return ZKP_ERR_ARG;
  if (n_msm == 0) return ZKP_OK;
  if (!off || !out || !status || off[0] != 0) return ZKP_ERR_ARG;
  for (uint32_t i = 0; i < n_msm; ++i)
    if (off[i + 1] < off[i]) return ZKP_ERR_ARG;
  const uint32_t T = off[n_msm];
  if (T && (!scalars || !points || n_points == 0)) return ZKP_ERR_ARG;
  if (!pidx && n_points != T) return ZKP_ERR_ARG;
  if (pidx)
    for (uint32_t t = 0; t < T; ++t)
      if (pidx[t] >= n_points) return ZKP_ERR_ARG;
  for (uint32_t i = 0; i < n_msm; ++i)
    if (off[i + 1] == off[i]) { std::memset(out + 32 * (size_t)i, 0, 32); status[i] = 0; }
  if (T == 0) return ZKP_OK;
  // stretches of equal numbers of terms, at least MIN_STRETCH each: a stretch pays the 256 doublings of its walks whatever its length
  constexpr uint32_t MIN_STRETCH = 16;
  unsigned t = n_threads > 0 ? (unsigned)n_threads : std::thread::hardware_concurrency();
  t = std::max(1u, std::min(std::min(t, 128u), (T + MIN_STRETCH - 1) / MIN_STRETCH));
  const uint32_t share = (uint32_t)(((uint64_t)T + t - 1) / t);
  std::vector<std::vector<SegPartial>> partials(t);
  auto work = [&](unsigned k) {
    const uint32_t lo = (uint32_t)std::min<uint64_t>(T, (uint64_t)k * share), hi = (uint32_t)std::min<uint64_t>(T, (uint64_t)lo + share);
    if (lo < hi) msm_stretch(lo, hi, n_msm, off, scalars, pidx, points, n_points, flags, out, status, partials[k]);
  };
  std::vector<std::thread> pool;
  for (unsigned k = 1; k < t; ++k) pool.emplace_back(work, k);
  work(0);
  for (std::thread& th : pool) th.join();
  // the cut segments: their partial sums lie in stretch order, those of one segment next to each other
  ge_p3 acc;
  bool bad = false, open = false;
  uint32_t seg = 0;
  auto finish = [&]() {
    status[seg] = bad ? 1 : 0;
    if (bad) std::memset(out + 32 * (size_t)seg, 0, 32);
    else encode(out + 32 * (size_t)seg, acc);
  };
  for (const auto& list : partials)
    for (const SegPartial& p : list) {
      if (open && p.seg != seg) { finish(); open = false; }
      if (!open) { ge_identity(acc); bad = false; seg = p.seg; open = true; }
      ge_cached c;
      ge_to_cached(c, p.sum);
      ge_add_cached(acc, acc, c);
      bad |= p.bad;
    }
  if (open) finish();
  return ZKP_OK;
}

int msm_optional(uint64_t n, const uint8_t* scalars, const uint8_t* points, uint8_t out_point[32], int* status) {
  if (!out_point || !status || (n && (!scalars || !points))) return ZKP_ERR_ARG;
  std::vector<Table> tabs(n);
  std::vector<int8_t> dig(65 * (n ? n : 1));
  std::vector<const Table*> tp(n);
  bool bad = false;
  for (uint64_t i = 0; i < n; ++i) {
    ge_p3 p;
    if (!decode(p, points + 32 * i)) { bad = true; break; }
    build_table(tabs[i], p);
    recode16(reinterpret_cast<int8_t(*)[65]>(dig.data())[i], scalars + 32 * i);
    tp[i] = &tabs[i];
  }
  std::memset(out_point, 0, 32);
  *status = bad ? 1 : 0;
  if (bad) return ZKP_OK;
  ge_p3 acc;
  straus<false>(acc, (size_t)n, reinterpret_cast<const int8_t(*)[65]>(dig.data()), tp.data());
  encode(out_point, acc);
  return ZKP_OK;
}

int decode_check(uint64_t n, const uint8_t* points, uint8_t* status) {
  if (n && (!points || !status)) return ZKP_ERR_ARG;
  for (uint64_t i = 0; i < n; ++i) {
    ge_p3 p;
    status[i] = decode(p, points + 32 * i) ? 0 : 1;
  }
  return ZKP_OK;
}

int from_uniform_bytes(uint64_t n, const uint8_t* in, uint8_t* out) {
  if (n && (!in || !out)) return ZKP_ERR_ARG;
  for (uint64_t i = 0; i < n; ++i) {
    ge_p3 p;
    ristretto_from_uniform_bytes(p, in + 64 * i);
    encode(out + 32 * i, p);
  }
  return ZKP_OK;
}

int hash_from_bytes_sha512(uint64_t n, const uint8_t* msgs, const uint64_t* offsets, uint8_t* out) {
  if (n && (!msgs || !offsets || !out)) return ZKP_ERR_ARG;
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t H[8];
    uint32_t w[16];
    sha512_range(H, msgs, offsets[n], offsets[i], offsets[i + 1]);
    sha512_digest_words(w, H);
    ge_p3 p;
    ristretto_from_uniform_words(p, w);
    encode(out + 32 * i, p);
  }
  return ZKP_OK;
}

// ---- scalars mod l: the bodies of k_sc_invert / k_sc_from_wide / k_sc_muladd / k_sc_hash_sha512 (element i0 + i of the call is i here) ----
namespace {
inline void sc_load(sc& r, const uint8_t* p) { std::memcpy(r.v, p, 32); }
inline void sc_store(uint8_t* p, const sc& a) { std::memcpy(p, a.v, 32); }
}  // namespace

void sc_invert_n(uint64_t n, const uint8_t* in, uint8_t* out) {
  for (uint64_t i = 0; i < n; ++i) {
    sc a, r;
    sc_load(a, in + 32 * i);
    sc_invert(r, a);
    sc_store(out + 32 * i, r);
  }
}

void sc_from_wide_n(uint64_t n, const uint8_t* in, uint8_t* out) {
  for (uint64_t i = 0; i < n; ++i) {
    sc lo, hi, r;
    sc_load(lo, in + 64 * i);
    sc_load(hi, in + 64 * i + 32);
    sc_from_wide(r, lo, hi);
    sc_store(out + 32 * i, r);
  }
}

void sc_muladd_n(uint64_t n, const uint8_t* a, uint32_t sa, const uint8_t* b, uint32_t sb, const uint8_t* c, uint32_t sc_, uint8_t* out) {
  for (uint64_t i = 0; i < n; ++i) {
    sc x, y, z, r;
    sc_load(x, a + 32 * i * sa);
    sc_load(y, b + 32 * i * sb);
    sc_zero(z);
    if (c) sc_load(z, c + 32 * i * sc_);
    sc_muladd(r, x, y, z);
    sc_store(out + 32 * i, r);
  }
}

// ---- segmented sums, products and dot products of scalars (zkp_mi355x.h (12)) ----
namespace {
struct ScPartial { uint32_t seg; sc v; };
// One thread's stretch [lo, hi) of the term axis, segment by segment.  A segment that lies wholly inside is finished here; the others leave a partial.
void sc_reduce_stretch(int op, uint32_t lo, uint32_t hi, uint32_t n_out, const uint32_t* off, const uint8_t* a, const uint32_t* aidx, const uint8_t* b,
                       const uint32_t* bidx, uint8_t* out, std::vector<ScPartial>& partials) {
  uint32_t s = (uint32_t)(std::upper_bound(off, off + n_out + 1, lo) - off) - 1;        // the segment of term lo
  for (; s < n_out && off[s] < hi; ++s) {
    const uint32_t t0 = std::max(off[s], lo), t1 = std::min(off[s + 1], hi);
    if (t0 >= t1) continue;                                                              // an empty segment inside the stretch
    sc acc;
    sc_zero(acc);
    acc.v[0] = op == ZKP_SC_PRODUCT ? 1u : 0u;
    for (uint32_t t = t0; t < t1; ++t) {
      sc x, y;
      sc_load(x, a + 32 * (size_t)(aidx ? aidx[t] : t));
      if (op == ZKP_SC_SUM) {
        sc_reduce(x, x);
        sc_add(acc, acc, x);
      } else if (op == ZKP_SC_PRODUCT) {
        sc_mul(acc, acc, x);
      } else {
        sc_load(y, b + 32 * (size_t)(bidx ? bidx[t] : t));
        sc_muladd(acc, x, y, acc);
      }
    }
    if (t0 == off[s] && t1 == off[s + 1]) sc_store(out + 32 * (size_t)s, acc);
    else partials.push_back({s, acc});
  }
}
}  // namespace

int sc_reduce_n(int op, uint32_t n_out, const uint32_t* off, const uint8_t* a, uint32_t n_a, const uint32_t* aidx, const uint8_t* b, uint32_t n_b,
                const uint32_t* bidx, int n_threads, uint8_t* out) {
  if (op != ZKP_SC_SUM && op != ZKP_SC_PRODUCT && op != ZKP_SC_DOT) return ZKP_ERR_ARG;
  if (op != ZKP_SC_DOT && (b || n_b || bidx)) return ZKP_ERR_ARG;
  if (n_out == 0) return ZKP_OK;
  if (!off || !out || off[0] != 0) return ZKP_ERR_ARG;
  for (uint32_t i = 0; i < n_out; ++i)
    if (off[i + 1] < off[i]) return ZKP_ERR_ARG;
  const uint32_t T = off[n_out];
  if (T > 0x7fffffffu) return ZKP_ERR_ARG;
  if (T && (!a || n_a == 0)) return ZKP_ERR_ARG;
  if (T && op == ZKP_SC_DOT && (!b || n_b == 0)) return ZKP_ERR_ARG;
  if (!aidx && n_a != T) return ZKP_ERR_ARG;
  if (op == ZKP_SC_DOT && !bidx && n_b != T) return ZKP_ERR_ARG;
  for (uint32_t t = 0; aidx && t < T; ++t)
    if (aidx[t] >= n_a) return ZKP_ERR_ARG;
  for (uint32_t t = 0; bidx && t < T; ++t)
    if (bidx[t] >= n_b) return ZKP_ERR_ARG;
  sc ident;
  sc_zero(ident);
  ident.v[0] = op == ZKP_SC_PRODUCT ? 1u : 0u;
  for (uint32_t i = 0; i < n_out; ++i)
    if (off[i + 1] == off[i]) sc_store(out + 32 * (size_t)i, ident);
  if (T == 0) return ZKP_OK;
  // stretches of equal numbers of terms, at least MIN_STRETCH each: a term is a few hundred instructions, starting a thread some microseconds
  constexpr uint32_t MIN_STRETCH = 64;
  unsigned nt = n_threads > 0 ? (unsigned)n_threads : std::thread::hardware_concurrency();
  nt = std::max(1u, std::min(std::min(nt, 128u), (T + MIN_STRETCH - 1) / MIN_STRETCH));
  const uint32_t share = (uint32_t)(((uint64_t)T + nt - 1) / nt);
  std::vector<std::vector<ScPartial>> partials(nt);
  auto work = [&](unsigned k) {
    const uint32_t lo = (uint32_t)std::min<uint64_t>(T, (uint64_t)k * share), hi = (uint32_t)std::min<uint64_t>(T, (uint64_t)lo + share);
    if (lo < hi) sc_reduce_stretch(op, lo, hi, n_out, off, a, aidx, b, bidx, out, partials[k]);
  };
  std::vector<std::thread> pool;
  for (unsigned k = 1; k < nt; ++k) pool.emplace_back(work, k);
  work(0);
  for (std::thread& th : pool) th.join();
  // the cut segments: their partials lie in stretch order, those of one segment next to each other
  sc acc;
  bool open = false;
  uint32_t seg = 0;
  for (const auto& list : partials)
    for (const ScPartial& p : list) {
      if (open && p.seg != seg) { sc_store(out + 32 * (size_t)seg, acc); open = false; }
      if (!open) { acc = ident; seg = p.seg; open = true; }
      if (op == ZKP_SC_PRODUCT) sc_mul(acc, acc, p.v);
      else sc_add(acc, acc, p.v);
    }
  if (open) sc_store(out + 32 * (size_t)seg, acc);
  return ZKP_OK;
}

// ---- segmented prefix sums and products of scalars, running sums of points (zkp_mi355x.h (13)) ----
namespace {
// Stretches of equal numbers of terms, at least 64 each (as sc_reduce_n cuts them): the number of stretches and the terms of one.
inline unsigned scan_stretches(uint32_t T, int n_threads, uint32_t& share) {
  constexpr uint32_t MIN_STRETCH = 64;
  unsigned nt = n_threads > 0 ? (unsigned)n_threads : std::thread::hardware_concurrency();
  nt = std::max(1u, std::min(std::min(nt, 128u), (T + MIN_STRETCH - 1) / MIN_STRETCH));
  share = (uint32_t)(((uint64_t)T + nt - 1) / nt);
  return nt;
}
template <typename F>
inline void scan_run(unsigned nt, F&& work) {
  std::vector<std::thread> pool;
  for (unsigned k = 1; k < nt; ++k) pool.emplace_back(work, k);
  work(0);
  for (std::thread& th : pool) th.join();
}
// the checks the two scans share, in the order of the engine's; T = off[n_seg] on success
inline int scan_check(uint32_t n_seg, const uint32_t* off, const void* rows, uint32_t n_rows, const uint32_t* idx, const void* out, uint32_t& T) {
  if (!off || off[0] != 0) return ZKP_ERR_ARG;
  for (uint32_t i = 0; i < n_seg; ++i)
    if (off[i + 1] < off[i]) return ZKP_ERR_ARG;
  T = off[n_seg];
  if (T > 0x7fffffffu) return ZKP_ERR_ARG;
  if (T && (!rows || n_rows == 0 || !out)) return ZKP_ERR_ARG;
  if (!idx && n_rows != T) return ZKP_ERR_ARG;
  for (uint32_t t = 0; idx && t < T; ++t)
    if (idx[t] >= n_rows) return ZKP_ERR_ARG;
  return ZKP_OK;
}
struct ScanStretch { uint32_t lo = 0, hi = 0, first_head = 0; };   // first_head: the first term of [lo, hi) that opens a segment, or hi
inline uint32_t sum_terms(ge_p3& acc, uint32_t lo, uint32_t hi, const uint32_t* pidx, const uint8_t* neg, const uint8_t* points);   // (below, with the sums)
}  // namespace

int sc_scan_n(int op, int mode, uint32_t n_seg, const uint32_t* off, const uint8_t* a, uint32_t n_a, const uint32_t* aidx, int n_threads, uint8_t* out) {
  if (op != ZKP_SC_SUM && op != ZKP_SC_PRODUCT) return ZKP_ERR_ARG;
  if (mode != ZKP_SCAN_INCLUSIVE && mode != ZKP_SCAN_EXCLUSIVE) return ZKP_ERR_ARG;
  if (n_seg == 0) return ZKP_OK;
  uint32_t T = 0;
  const int rc = scan_check(n_seg, off, a, n_a, aidx, out, T);
  if (rc || T == 0) return rc;
  const bool mul = op == ZKP_SC_PRODUCT, excl = mode == ZKP_SCAN_EXCLUSIVE;
  sc ident;
  sc_zero(ident);
  ident.v[0] = mul ? 1u : 0u;
  uint32_t share = 0;
  const unsigned nt = scan_stretches(T, n_threads, share);
  std::vector<ScanStretch> st(nt);
  std::vector<sc> total(nt, ident), carry(nt, ident);
  // every thread scans its stretch from the identity; what is open at its end is its total
  scan_run(nt, [&](unsigned k) {
    ScanStretch& z = st[k];
    z.lo = (uint32_t)std::min<uint64_t>(T, (uint64_t)k * share);
    z.hi = (uint32_t)std::min<uint64_t>(T, (uint64_t)z.lo + share);
    z.first_head = z.hi;
    if (z.lo >= z.hi) return;
    uint32_t s = (uint32_t)(std::upper_bound(off, off + n_seg + 1, z.lo) - off) - 1;      // the segment of term lo
    sc acc = ident;
    for (uint32_t t = z.lo; t < z.hi; ++t) {
      while (t >= off[s + 1]) ++s;
      if (t == off[s]) {
        acc = ident;
        if (z.first_head == z.hi) z.first_head = t;
      }
      if (excl) sc_store(out + 32 * (size_t)t, acc);
      sc x;
      sc_load(x, a + 32 * (size_t)(aidx ? aidx[t] : t));
      if (mul) {
        sc_mul(acc, acc, x);
      } else {
        sc_reduce(x, x);
        sc_add(acc, acc, x);
      }
      if (!excl) sc_store(out + 32 * (size_t)t, acc);
    }
    total[k] = acc;
  });
  // the stretch totals, scanned serially: carry[k] is what is open where stretch k begins
  sc c = ident;
  for (unsigned k = 0; k < nt; ++k) {
    carry[k] = c;
    if (st[k].lo >= st[k].hi) continue;
    if (st[k].first_head != st[k].hi) c = total[k];
    else if (mul) sc_mul(c, c, total[k]);
    else sc_add(c, c, total[k]);
  }
  // every thread fixes up its first run
  scan_run(nt, [&](unsigned k) {
    if (k == 0) return;
    for (uint32_t t = st[k].lo; t < st[k].first_head; ++t) {
      sc x;
      sc_load(x, out + 32 * (size_t)t);
      if (mul) sc_mul(x, carry[k], x);
      else sc_add(x, carry[k], x);
      sc_store(out + 32 * (size_t)t, x);
    }
  });
  return ZKP_OK;
}

int point_scan_n(int mode, uint32_t n_seg, const uint32_t* off, const uint32_t* pidx, const uint8_t* neg, const uint8_t* points, uint32_t n_points, int n_threads,
                 uint8_t* out, uint8_t* status) {
  if (mode != ZKP_SCAN_INCLUSIVE && mode != ZKP_SCAN_EXCLUSIVE) return ZKP_ERR_ARG;
  if (n_seg == 0) return ZKP_OK;
  uint32_t T = 0;
  const int rc = scan_check(n_seg, off, points, n_points, pidx, out, T);
  if (rc || T == 0) return rc;
  if (!status) return ZKP_ERR_ARG;
  const bool excl = mode == ZKP_SCAN_EXCLUSIVE;
  uint32_t share = 0;
  const unsigned nt = scan_stretches(T, n_threads, share);
  std::vector<ScanStretch> st(nt);
  std::vector<ge_p3> total(nt), carry(nt);
  std::vector<uint32_t> total_bad(nt, 0), carry_bad(nt, 0);
  // rows [from, to), the walk starting at `from` with (acc, bad).  after_head: only the rows from the first head on are written (the others wait
  // for their carry).  first_head: the first term of the range that opens a segment, or `to`.
  auto walk = [&](uint32_t from, uint32_t to, bool after_head, ge_p3& acc, uint32_t& bad, uint32_t& first_head) {
    uint32_t s = (uint32_t)(std::upper_bound(off, off + n_seg + 1, from) - off) - 1;      // the segment of term `from`
    first_head = to;
    auto put = [&](uint32_t t) {
      if (after_head && first_head == to) return;
      status[t] = (uint8_t)bad;
      if (bad) std::memset(out + 32 * (size_t)t, 0, 32);
      else encode(out + 32 * (size_t)t, acc);
    };
    for (uint32_t t = from; t < to; ++t) {
      while (t >= off[s + 1]) ++s;
      if (t == off[s]) {
        ge_identity(acc);
        bad = 0;
        if (first_head == to) first_head = t;
      }
      if (excl) put(t);
      bad |= sum_terms(acc, t, t + 1, pidx, neg, points);
      if (!excl) put(t);
    }
  };
  // every thread walks its stretch from the identity: the rows from its first head on are final, what is open at its end is its total
  scan_run(nt, [&](unsigned k) {
    ScanStretch& z = st[k];
    z.lo = (uint32_t)std::min<uint64_t>(T, (uint64_t)k * share);
    z.hi = (uint32_t)std::min<uint64_t>(T, (uint64_t)z.lo + share);
    z.first_head = z.hi;
    ge_identity(total[k]);
    if (z.lo < z.hi) walk(z.lo, z.hi, true, total[k], total_bad[k], z.first_head);
  });
  ge_p3 c;
  ge_identity(c);
  uint32_t cbad = 0;
  for (unsigned k = 0; k < nt; ++k) {
    carry[k] = c;
    carry_bad[k] = cbad;
    if (st[k].lo >= st[k].hi) continue;
    if (st[k].first_head != st[k].hi) {
      c = total[k];
      cbad = total_bad[k];
    } else {
      ge_cached q;
      ge_to_cached(q, total[k]);
      ge_add_cached(c, c, q);
      cbad |= total_bad[k];
    }
  }
  // every thread walks its first run again, from its carry
  scan_run(nt, [&](unsigned k) {
    if (k == 0 || st[k].lo >= st[k].first_head) return;
    uint32_t none;
    walk(st[k].lo, st[k].first_head, false, carry[k], carry_bad[k], none);
  });
  return ZKP_OK;
}

void sc_hash_sha512_n(uint64_t n, const uint8_t* msgs, const uint64_t* offsets, uint8_t* out) {
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t H[8];
    uint32_t w[16];
    sha512_range(H, msgs, offsets[n], offsets[i], offsets[i + 1]);
    sha512_digest_words(w, H);
    sc lo, hi, r;
    for (int k = 0; k < 8; ++k) { lo.v[k] = w[k]; hi.v[k] = w[8 + k]; }
    sc_from_wide(r, lo, hi);
    sc_store(out + 32 * i, r);
  }
}

// ---- Scalar * basepoint, Scalar * point (zkp_mi355x.h (8)): one Straus walk per output over the point's table {1..8} P ----
namespace {
const uint8_t kBasepoint[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f,
                                0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
template <bool CT>
inline void mul_one(uint8_t* out, const uint8_t* scalar, const Table& t) {
  int8_t dig[1][65];
  recode16(dig[0], scalar);
  const Table* tp[1] = {&t};
  ge_p3 acc;
  straus<CT>(acc, 1, dig, tp);
  encode(out, acc);
}
}  // namespace

void mul_base_n(uint64_t n, const uint8_t* scalars, uint8_t* out) {
  if (n == 0) return;
  ge_p3 b;
  decode(b, kBasepoint);
  Table t;
  build_table(t, b);
  for (uint64_t i = 0; i < n; ++i) mul_one<true>(out + 32 * i, scalars + 32 * i, t);
}

void mul_points_n(uint64_t n, const uint8_t* scalars, uint32_t ss, const uint8_t* points, uint32_t ps, int flags, uint8_t* out, uint8_t* status) {
  Table t;
  uint32_t good = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (i == 0 || ps) {                                              // (a shared point is decoded and tabulated once)
      ge_p3 p;
      good = decode(p, points + 32 * i * ps);                        // before out[i] is written: out may be points
      if (good) build_table(t, p);
    }
    status[i] = good ? 0 : 1;
    if (!good) { std::memset(out + 32 * i, 0, 32); continue; }
    if (flags == ZKP_CT) mul_one<true>(out + 32 * i, scalars + 32 * i * ss, t);
    else mul_one<false>(out + 32 * i, scalars + 32 * i * ss, t);
  }
}

// ---- RistrettoPoint sums (zkp_mi355x.h (9)) ----
void add_points_n(uint64_t n, const uint8_t* a, uint32_t as, const uint8_t* b, uint32_t bs, int op, uint8_t* out, uint8_t* status) {
  ge_p3 pa, pb;
  ge_cached qb;
  uint32_t ok_a = 0, ok_b = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (i == 0 || as) ok_a = decode(pa, a + 32 * i * as);            // both before out[i] is written: out may be a or b
    if (i == 0 || bs) {
      ok_b = decode(pb, b + 32 * i * bs);
      ge_to_cached(qb, pb);
      ge_cached_cneg(qb, (uint32_t)(op == ZKP_PT_SUB));
    }
    status[i] = (ok_a & ok_b) ? 0 : 1;
    if (!(ok_a & ok_b)) { std::memset(out + 32 * i, 0, 32); continue; }
    ge_p3 r;
    ge_add_cached(r, pa, qb);
    encode(out + 32 * i, r);
  }
}

namespace {
// acc += +- decode(points[pidx[t]]) for t in [lo, hi); returns 1 if a point did not decode (such a point adds the identity)
inline uint32_t sum_terms(ge_p3& acc, uint32_t lo, uint32_t hi, const uint32_t* pidx, const uint8_t* neg, const uint8_t* points) {
  uint32_t bad = 0;
  for (uint32_t t = lo; t < hi; ++t) {
    ge_p3 p;
    ge_cached q;
    bad |= decode(p, points + 32 * (size_t)(pidx ? pidx[t] : t)) ^ 1u;
    ge_to_cached(q, p);
    ge_cached_cneg(q, (uint32_t)(neg && neg[t]));
    ge_add_cached(acc, acc, q);
  }
  return bad;
}
}  // namespace

void sum_points_n(uint32_t n_sums, const uint32_t* off, const uint32_t* pidx, const uint8_t* neg, const uint8_t* points, uint8_t* out, uint8_t* status,
                  uint32_t skip_longer_than) {
  for (uint32_t i = 0; i < n_sums; ++i) {
    if (off[i + 1] - off[i] > skip_longer_than) continue;
    ge_p3 acc;
    ge_identity(acc);
    const uint32_t bad = sum_terms(acc, off[i], off[i + 1], pidx, neg, points);
    status[i] = (uint8_t)bad;
    if (bad) std::memset(out + 32 * (size_t)i, 0, 32);
    else encode(out + 32 * (size_t)i, acc);
  }
}

void sum_points_partial(uint32_t t_lo, uint32_t t_hi, const uint32_t* pidx, const uint8_t* neg, const uint8_t* points, uint8_t partial[SUM_PARTIAL_BYTES]) {
  ge_p3 acc;
  ge_identity(acc);
  partial[128] = (uint8_t)sum_terms(acc, t_lo, t_hi, pidx, neg, points);
  const fe* co[4] = {&acc.X, &acc.Y, &acc.Z, &acc.T};
  for (int k = 0; k < 4; ++k) {
    uint32_t w[8];
    fe_towords(w, *co[k]);
    std::memcpy(partial + 32 * k, w, 32);
  }
}

void sum_points_finish(uint32_t n, const uint8_t* partials, uint8_t out[32], uint8_t* status) {
  ge_p3 acc;
  ge_identity(acc);
  uint32_t bad = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t* p = partials + SUM_PARTIAL_BYTES * (size_t)i;
    ge_p3 q;
    fe* co[4] = {&q.X, &q.Y, &q.Z, &q.T};
    for (int k = 0; k < 4; ++k) {
      uint32_t w[8];
      std::memcpy(w, p + 32 * k, 32);
      fe_fromwords(*co[k], w);
    }
    bad |= p[128];
    ge_cached c;
    ge_to_cached(c, q);
    ge_add_cached(acc, acc, c);
  }
  *status = (uint8_t)(bad != 0);
  if (bad) std::memset(out, 0, 32);
  else encode(out, acc);
}

// ---- bounded discrete logarithms to the basepoint (zkp_mi355x.h (10); dlog.h has the scheme) ----
namespace {
inline void mul_p3(ge_p3& r, const uint8_t scalar[32], const ge_p3& p) {
  Table t;
  build_table(t, p);
  int8_t dig[1][65];
  recode16(dig[0], scalar);
  const Table* tp[1] = {&t};
  straus<false>(r, 1, dig, tp);
}
inline void small_scalar(uint8_t s[32], uint64_t v) {
  std::memset(s, 0, 32);
  std::memcpy(s, &v, 8);
}
inline void half_scalar(uint8_t s[32]) {             // (l + 1) / 2 = 1 / 2 mod l
  uint32_t w[8];
  for (int i = 0; i < 8; ++i) w[i] = sc_half(i);
  w[0] += 1u;
  std::memcpy(s, w, 32);
}

// w[i] = encode(2 cand[i]) for i < g from ONE inversion.  x = 0 (the double is the identity) is replaced by 1 with a select and the bytes by the
// identity's encoding: the product of the group never vanishes.
struct DoubleEncoder {
  std::vector<ristretto_dc_state> st;
  std::vector<fe> x, pre;
  std::vector<uint32_t> zero;
  void run(uint32_t (*w)[8], const ge_p3* cand, size_t g) {
    st.resize(g); x.resize(g); pre.resize(g); zero.resize(g);
    fe one;
    fe_1(one);
    for (size_t i = 0; i < g; ++i) {
      ristretto_dc_prepare(st[i], x[i], cand[i]);
      zero[i] = fe_iszero(x[i]);
      fe_cmov(x[i], one, zero[i]);
      if (i == 0) pre[0] = x[0];
      else fe_mul(pre[i], pre[i - 1], x[i]);
    }
    fe inv;
    fe_invert(inv, pre[g - 1]);
    for (size_t i = g; i-- > 0;) {
      fe mine;
      if (i) { fe_mul(mine, inv, pre[i - 1]); fe_mul(inv, inv, x[i]); }
      else mine = inv;
      ristretto_dc_finish(w[i], st[i], mine);
      for (int k = 0; k < 8; ++k) w[i][k] = zero[i] ? 0u : w[i][k];
    }
  }
};

struct DlogTable {
  uint32_t baby_bits = 0;
  uint8_t enc[32] = {};                              // the base's encoding (the cache's key with baby_bits)
  std::vector<uint32_t> rows;
  std::vector<dlog_slot> slots;
  ge_p3 base;
  ge_cached step;                                    // (m / 2) G
  ge_cached group_step;                              // DLOG_GROUP (m / 2) G: from the first candidate of one group to that of the next
  uint64_t used = 0;
};

void build_dlog_table(DlogTable& t, const ge_p3& base, uint32_t baby_bits) {
  const uint32_t m = 1u << baby_bits;
  t.baby_bits = baby_bits;
  t.base = base;
  uint8_t s[32];
  ge_p3 hb, sp;
  half_scalar(s);
  mul_p3(hb, s, t.base);
  ge_cached half_b;
  ge_to_cached(half_b, hb);
  small_scalar(s, m / 2);
  mul_p3(sp, s, t.base);
  ge_to_cached(t.step, sp);
  small_scalar(s, (uint64_t)(m / 2) * DLOG_GROUP);
  mul_p3(sp, s, t.base);
  ge_to_cached(t.group_step, sp);
  t.rows.resize((size_t)m * 8);
  DoubleEncoder enc;
  std::vector<ge_p3> cand(DLOG_GROUP);
  ge_p3 P;
  ge_identity(P);
  for (uint32_t i0 = 0; i0 < m; i0 += DLOG_GROUP) {
    const size_t g = std::min<uint32_t>(DLOG_GROUP, m - i0);
    for (size_t i = 0; i < g; ++i) {
      cand[i] = P;
      ge_add_cached(P, P, half_b);
    }
    enc.run(reinterpret_cast<uint32_t(*)[8]>(t.rows.data() + 8 * (size_t)i0), cand.data(), g);
  }
  t.slots.assign(dlog_slot_count(baby_bits), dlog_slot{0u, 0u});
  dlog_fill_slots(t.slots.data(), t.rows.data(), baby_bits);
}

// the table of (base, baby_bits), built at its first use; NULL where the base does not decode.  At most DLOG_POINT_SLOTS tables are kept, the
// least recently used one leaves (callers that still search it hold their own reference).
std::shared_ptr<const DlogTable> dlog_table(const uint8_t base[32], uint32_t baby_bits) {
  static std::mutex mu;
  static std::vector<std::shared_ptr<DlogTable>> tables;
  static uint64_t tick = 0;
  std::lock_guard<std::mutex> lk(mu);
  for (auto& t : tables)
    if (t->baby_bits == baby_bits && std::memcmp(t->enc, base, 32) == 0) {
      t->used = ++tick;
      return t;
    }
  ge_p3 G;
  if (!decode(G, base)) return nullptr;
  auto t = std::make_shared<DlogTable>();
  build_dlog_table(*t, G, baby_bits);
  std::memcpy(t->enc, base, 32);
  t->used = ++tick;
  if (tables.size() >= DLOG_POINT_SLOTS) {
    size_t lru = 0;
    for (size_t i = 1; i < tables.size(); ++i)
      if (tables[i]->used < tables[lru]->used) lru = i;
    tables[lru] = t;
  } else {
    tables.push_back(t);
  }
  return t;
}

inline void half_store(uint8_t half[DLOG_HALF_BYTES], const ge_p3& P) {
  const fe* co[4] = {&P.X, &P.Y, &P.Z, &P.T};
  for (int k = 0; k < 4; ++k) {
    uint32_t w[8];
    fe_towords(w, *co[k]);
    std::memcpy(half + 32 * k, w, 32);
  }
}
inline void half_load(ge_p3& P, const uint8_t half[DLOG_HALF_BYTES]) {
  fe* co[4] = {&P.X, &P.Y, &P.Z, &P.T};
  for (int c = 0; c < 4; ++c) {
    uint32_t w[8];
    std::memcpy(w, half + 32 * c, 32);
    fe_fromwords(*co[c], w);
  }
}
}  // namespace

bool dlog_point_decodes(const uint8_t base[32]) {
  ge_p3 G;
  return decode(G, base);
}
int dlog_point_prepare_table(const uint8_t base[32], uint32_t baby_bits) { return dlog_table(base, baby_bits) ? 0 : ZKP_DLOG_INVALID; }
void dlog_prepare_table(uint32_t baby_bits) { (void)dlog_table(kBasepoint, baby_bits); }

void dlog_point_shift(const uint8_t base[32], uint32_t bits, uint8_t shift[DLOG_HALF_BYTES]) {
  ge_p3 G, S;
  uint8_t s[32];
  if (!decode(G, base)) ge_identity(G);
  if (bits >= 2) small_scalar(s, 1ull << (bits - 2));                  // 2^(bits - 1) / 2
  else half_scalar(s);                                                 // bits = 1: (1/2) G
  mul_p3(S, s, G);
  half_store(shift, S);
}

int dlog_point_halve(const uint8_t point[32], const uint8_t* shift, uint8_t half[DLOG_HALF_BYTES]) {
  ge_p3 Q, P;
  if (!decode(Q, point)) {
    std::memset(half, 0, DLOG_HALF_BYTES);
    return ZKP_DLOG_INVALID;
  }
  uint8_t s[32];
  half_scalar(s);
  mul_p3(P, s, Q);                                   // Q / 2: every candidate of the search is a half, its bytes come from the encoder of doubles
  if (shift) {
    ge_p3 S;
    ge_cached cs;
    half_load(S, shift);
    ge_to_cached(cs, S);
    ge_add_cached(P, P, cs);
  }
  half_store(half, P);
  return ZKP_DLOG_NOT_FOUND;
}
int dlog_halve(const uint8_t point[32], uint8_t half[DLOG_HALF_BYTES]) { return dlog_point_halve(point, nullptr, half); }

int dlog_point_range(const uint8_t base[32], const uint8_t half[DLOG_HALF_BYTES], uint32_t bits, uint32_t baby_bits, bool is_signed, uint64_t j_lo,
                     uint64_t j_hi, uint64_t* k) {
  *k = 0;
  const std::shared_ptr<const DlogTable> tab = dlog_table(base, baby_bits);
  if (!tab || j_lo >= j_hi) return ZKP_DLOG_NOT_FOUND;
  const DlogTable& t = *tab;
  // Groups of DLOG_GROUP giant steps, numbered over the whole range of the call; this range holds [g_lo, g_hi), the first and the last of them
  // in part where j_lo or j_hi is no multiple of the group.  The order visits the groups above its first one in ascending and those below it in
  // descending order, so two cursors follow it: `up` stands on the next candidate going up and simply walks on, `down` on the first candidate of
  // group g_down - 1 and moves by one addition per group.
  const uint64_t n_groups = (dlog_giant_steps(bits, baby_bits) + DLOG_GROUP - 1) / DLOG_GROUP;
  const uint64_t g_lo = j_lo / DLOG_GROUP, g_hi = (j_hi + DLOG_GROUP - 1) / DLOG_GROUP;
  uint64_t g_up = std::min(std::max(dlog_slice_order(n_groups, is_signed, 0), g_lo), g_hi), g_down = g_up;
  ge_p3 up, down;
  half_load(up, half);
  if (g_up || j_lo) {                                // (above g_lo the start is the group's own; in g_lo it is j_lo)
    uint8_t s[32];
    ge_p3 A;
    ge_cached ca;
    small_scalar(s, std::max(g_up * DLOG_GROUP, j_lo) << (baby_bits - 1u));
    mul_p3(A, s, t.base);
    ge_to_cached(ca, A);
    ge_sub_cached(up, up, ca);
  }
  ge_add_cached(down, up, t.group_step);
  const uint64_t bias = is_signed ? 1ull << (bits - 1) : 0ull;
  DoubleEncoder enc;
  std::vector<ge_p3> cand(DLOG_GROUP);
  std::vector<uint32_t> w((size_t)DLOG_GROUP * 8);
  for (uint64_t i = 0; i < n_groups && (g_up < g_hi || g_down > g_lo); ++i) {
    const uint64_t g = dlog_slice_order(n_groups, is_signed, i);
    if (g < g_lo || g >= g_hi) continue;
    const bool going_up = g == g_up;                 // (else g == g_down - 1)
    const uint64_t j0 = std::max(g * DLOG_GROUP, j_lo);
    ge_p3 P;
    if (going_up) {
      P = up;
    } else {
      P = down;
      ge_add_cached(down, down, t.group_step);
      --g_down;
      for (uint64_t j = g * DLOG_GROUP; j < j0; ++j) ge_sub_cached(P, P, t.step);
    }
    const size_t n = (size_t)(std::min<uint64_t>((g + 1) * DLOG_GROUP, j_hi) - j0);
    for (size_t c = 0; c < n; ++c) {
      cand[c] = P;
      ge_sub_cached(P, P, t.step);
    }
    if (going_up) {
      up = P;
      ++g_up;
    }
    enc.run(reinterpret_cast<uint32_t(*)[8]>(w.data()), cand.data(), n);
    for (size_t c = 0; c < n; ++c) {
      const uint32_t b = dlog_probe(w.data() + 8 * c, t.slots.data(), t.rows.data(), baby_bits);
      const uint64_t v = ((j0 + c) << baby_bits) + b;
      if (b != DLOG_NONE && dlog_in_range(v, bits)) {
        *k = v - bias;
        return ZKP_DLOG_FOUND;
      }
    }
  }
  return ZKP_DLOG_NOT_FOUND;
}
int dlog_base_range(const uint8_t half[DLOG_HALF_BYTES], uint32_t bits, uint32_t baby_bits, uint64_t j_lo, uint64_t j_hi, uint64_t* k) {
  return dlog_point_range(kBasepoint, half, bits, baby_bits, false, j_lo, j_hi, k);
}

void dlog_point_n(const uint8_t base[32], uint64_t n, const uint8_t* points, uint32_t bits, uint32_t baby_bits, bool is_signed, uint64_t* out,
                  uint8_t* status) {
  const uint64_t J = dlog_giant_steps(bits, baby_bits);
  uint8_t shift[DLOG_HALF_BYTES];
  if (is_signed) dlog_point_shift(base, bits, shift);
  for (uint64_t i = 0; i < n; ++i) {
    uint8_t half[DLOG_HALF_BYTES];
    out[i] = 0;
    status[i] = (uint8_t)dlog_point_halve(points + 32 * i, is_signed ? shift : nullptr, half);
    if (status[i] != ZKP_DLOG_INVALID) status[i] = (uint8_t)dlog_point_range(base, half, bits, baby_bits, is_signed, 0, J, out + i);
  }
}
void dlog_base_n(uint64_t n, const uint8_t* points, uint32_t bits, uint32_t baby_bits, uint64_t* out, uint8_t* status) {
  dlog_point_n(kBasepoint, n, points, bits, baby_bits, false, out, status);
}

}  // namespace hostbk
}  // namespace zkp
