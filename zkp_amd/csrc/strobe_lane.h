// One-lane STROBE-128 and the two Merlin operations every flow starts from, for the host and the device: append_message and
// challenge_bytes on ONE transcript whose position is only known at run time (host/merlin.cpp:61-150 restated; merlin_prog.h compiles
// programs for batches whose positions the host knows, this header needs no program).
//
// g++ (the stand-alone drivers tests/host/transcript_ops_host_main.cpp and transcript_rng_host_main.cpp, and the host library's
// host/transcript_rng.cpp) and hipcc compile the same text.  The 25 state words are a strided
// column, S[i * stride]: an LDS column per lane on the device (a run-time position indexes LDS, never a register array: no scratch),
// stride 1 on the host.  The permutation is merlin_prog.h's one-lane Keccak-f[1600] (tr_keccak_f).
//
// Bytes move in steps of up to 8: a step ends at the end of its state word, of the 166-byte block or of its input, whichever comes
// first, so that after the first step of a run every step is a whole state word (the shift-and-mask of tr_exec_op).
//
// A Merlin operation is one stream of five parts -- header of meta_ad, label, u32le(len), header of ad / prf, data -- which
// strobe_merlin_op walks in ONE loop:   consume up to the block boundary;  run_f at one place;  repeat while input is left.
// Lanes of a wavefront stand at different positions and hold different lengths; with the permutation outside the per-step loop a
// wavefront runs max over its lanes of the lane's permutation count, not their sum.
// Branches and addresses depend on positions, label lengths and data lengths only, never on message or state bytes.
//
// The second half of the header is the part walker (strobe_walk): the same loop over ANY sequence of parts, among them KEY (flags A|C:
// it overwrites where ad XORs), the two frames of Merlin's TranscriptRng that strobe_merlin_op does not walk -- meta_ad("rng") without a
// length, fill_bytes with a length and no label -- and a 64-byte PRF reduced mod l in the lane (sc25519.h).  On it stand the witness RNG
// (TranscriptRng: build_rng, rekey_with_witness_bytes, finalize, fill_bytes / Scalar::random), get_challenge and the point appends of the
// reference's TranscriptProtocol (src/toolbox/mod.rs:165-228).
#pragma once
#include <stdint.h>
#include "merlin_prog.h"   // ZKP_HD, tr_keccak_f, tr_bytemask
#include "sha512.h"        // sha512_clamp
#include "sc25519.h"       // sc_reduce_wide

namespace zkp {

constexpr uint32_t STROBE_RATE = 166;
constexpr uint32_t STROBE_I = 1, STROBE_A = 2, STROBE_C = 4, STROBE_M = 16;    // the flags Merlin uses: KEY is A|C (K and T never appear)

// A label as a kernel argument: its bytes in little-endian words, zero padded.  One word stays free behind the last label byte, so
// that the unaligned 8-byte fetch may read word k + 1.
constexpr uint32_t STROBE_LABEL_WORDS = 32;
constexpr uint32_t STROBE_LABEL_MAX = 8 * (STROBE_LABEL_WORDS - 1);
struct strobe_label {
  uint32_t len, reserved;
  uint64_t w[STROBE_LABEL_WORDS];
};
// false: the label is longer than STROBE_LABEL_MAX bytes
inline bool strobe_label_pack(strobe_label& l, const char* label, size_t n) {
  memset(&l, 0, sizeof(l));
  if (n > STROBE_LABEL_MAX) return false;
  l.len = (uint32_t)n;
  memcpy(l.w, label, n);      // (little-endian host)
  return true;
}

// One transcript: the state column and the three trailing bytes of its 208-byte blob (ZKP_TRANSCRIPT_BYTES).
struct strobe_lane {
  uint64_t* S;
  int stride;
  uint32_t pos, pos_begin, cur_flags;
};

// blob -> lane.  Returns the blob's word 25 as it stands; a position byte >= STROBE_RATE marks a corrupt blob, which the callers pass
// through untouched (no operation below may run on it: pos indexes the column).
ZKP_HD uint64_t strobe_load(strobe_lane& L, const uint64_t* blob) {
#pragma unroll
  for (int i = 0; i < 25; ++i) L.S[i * L.stride] = blob[i];
  const uint64_t tail = blob[25];
  L.pos = (uint32_t)tail & 0xffu;
  L.pos_begin = (uint32_t)(tail >> 8) & 0xffu;
  L.cur_flags = (uint32_t)(tail >> 16) & 0xffu;
  return tail;
}
ZKP_HD bool strobe_valid(const strobe_lane& L) { return L.pos < STROBE_RATE; }
ZKP_HD uint64_t strobe_tail(const strobe_lane& L) { return (uint64_t)(L.pos | L.pos_begin << 8 | L.cur_flags << 16); }   // the 5 padding bytes are zeros
ZKP_HD void strobe_store(const strobe_lane& L, uint64_t* blob, uint64_t tail) {
#pragma unroll
  for (int i = 0; i < 25; ++i) blob[i] = L.S[i * L.stride];
  blob[25] = tail;
}

// Strobe128::run_f
ZKP_HD void strobe_run_f(strobe_lane& L) {
  const uint32_t p = L.pos, q = p + 1;                                            // p <= 166: bytes p and p + 1 lie in words 0..20
  L.S[(p >> 3) * L.stride] ^= (uint64_t)L.pos_begin << (8 * (p & 7));
  L.S[(q >> 3) * L.stride] ^= 0x04ULL << (8 * (q & 7));
  L.S[20 * L.stride] ^= 0x80ULL << 56;                                            // byte 167 = kRate + 1
  tr_keccak_f(L.S, L.stride);
  L.pos = 0;
  L.pos_begin = 0;
}

// Strobe128::begin_op(flags, more = false) up to its header: the two header bytes {old pos_begin, flags} as a little-endian value, which
// the caller absorbs.  The run_f that follows the header of an operation with the C flag is the caller's too (strobe_merlin_op).
ZKP_HD uint64_t strobe_begin_op(strobe_lane& L, uint32_t flags) {
  const uint64_t hdr = L.pos_begin | flags << 8;
  L.pos_begin = L.pos + 1;
  L.cur_flags = flags;
  return hdr;
}

// the bytes one step moves at pos (< STROBE_RATE) when rem are left: 1..8, or 0 for rem = 0
ZKP_HD uint32_t strobe_step(uint32_t pos, uint64_t rem) {
  uint32_t nb = 8 - (pos & 7);
  nb = nb < STROBE_RATE - pos ? nb : STROBE_RATE - pos;
  return rem < nb ? (uint32_t)rem : nb;
}
// Strobe128::absorb of the low nb bytes of x, nb = strobe_step(pos, ..): they stay inside one state word and inside the block
ZKP_HD void strobe_absorb_step(strobe_lane& L, uint64_t x, uint32_t nb) {
  L.S[(L.pos >> 3) * L.stride] ^= (x & tr_bytemask(nb)) << (8 * (L.pos & 7));
  L.pos += nb;
}
// Strobe128::squeeze of nb bytes, nb = strobe_step(pos, ..): returns them, zeroes them in the state
ZKP_HD uint64_t strobe_squeeze_step(strobe_lane& L, uint32_t nb) {
  const uint32_t b = 8 * (L.pos & 7);
  const uint64_t m = tr_bytemask(nb), w = L.S[(L.pos >> 3) * L.stride];
  L.S[(L.pos >> 3) * L.stride] = w & ~(m << b);
  L.pos += nb;
  return (w >> b) & m;
}

// label bytes [off, off + 8) (off < len <= STROBE_LABEL_MAX), the bytes past the label as they come
ZKP_HD uint64_t strobe_label_fetch(const uint64_t* lab, uint32_t off) {
  const uint32_t k = off >> 3, s = 8 * (off & 7);
  uint64_t x = lab[k] >> s;
  if (s) x |= lab[k + 1] << (64 - s);
  return x;
}

// The bytes m[0, len) of a message as a source: get(off) = bytes [off, off + 8) little-endian, for off < len; the bytes at or past len
// hold anything (the step masks them).
//   host:   byte loads, each of a byte of the message.
//   device: aligned dword loads funnel-shifted by the byte offset, as sha512_range reads.  A dword is loaded only if it holds a byte of
//           the message, so no load reaches an aligned dword outside the buffer the message lies in; m may have any alignment.
struct strobe_msg {
  const uint8_t* m;
  uint64_t len;
  ZKP_HD uint64_t get(uint64_t off) const {
#ifdef __HIP_DEVICE_COMPILE__
    const uintptr_t a = reinterpret_cast<uintptr_t>(m) + off, end = reinterpret_cast<uintptr_t>(m) + len;
    const uint32_t sh = (uint32_t)(a & 3);
    const uint32_t* d = reinterpret_cast<const uint32_t*>(a - sh);
    const uint32_t d0 = d[0];                                                  // holds byte off < len
    const uint32_t d1 = reinterpret_cast<uintptr_t>(d + 1) < end ? d[1] : 0u;
    const uint32_t d2 = reinterpret_cast<uintptr_t>(d + 2) < end ? d[2] : 0u;
    return (uint64_t)__builtin_amdgcn_alignbit(d2, d1, 8 * sh) << 32 | __builtin_amdgcn_alignbit(d1, d0, 8 * sh);
#else
    uint64_t x = 0;
    for (int k = 0; k < 8; ++k)
      if (off + k < len) x |= (uint64_t)m[off + k] << (8 * k);
    return x;
#endif
  }
};
// The bytes d[0, len) of a PRF output as a sink: put(off, e, nb) writes the low nb bytes of e at d + off, d of any alignment
struct strobe_out {
  uint8_t* d;
  ZKP_HD void put(uint64_t off, uint64_t e, uint32_t nb) const {
    uint8_t* p = d + off;
    const uint32_t al = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 7);
    if (nb == 8 && al == 0) {
      __builtin_memcpy(__builtin_assume_aligned(p, 8), &e, 8);
    } else if (nb == 8 && al == 4) {
      const uint32_t lo = (uint32_t)e, hi = (uint32_t)(e >> 32);
      __builtin_memcpy(__builtin_assume_aligned(p, 4), &lo, 4);
      __builtin_memcpy(__builtin_assume_aligned(p + 4, 4), &hi, 4);
    } else {
      for (uint32_t i = 0; i < nb; ++i) p[i] = (uint8_t)(e >> (8 * i));
    }
  }
};

// meta_ad(label, more = false); meta_ad(u32le(frame_len), more = true); then
//   SQUEEZE = false:  ad(io[0, data_len), more = false)            -- Transcript::append_message
//   SQUEEZE = true:   prf(io[0, data_len), more = false)           -- Transcript::challenge_bytes: prf carries the C flag, so its
//                                                                     begin_op runs the permutation when pos != 0
// on a valid lane (strobe_valid).  lab = the label's words (strobe_label::w or a copy), lab_len <= STROBE_LABEL_MAX.
template <bool SQUEEZE, class Io>
ZKP_HD void strobe_merlin_op(strobe_lane& L, const uint64_t* lab, uint32_t lab_len, uint32_t frame_len, uint64_t data_len, const Io& io) {
  enum : uint32_t { P_HDR0, P_LABEL, P_LEN, P_HDR1, P_DATA, P_END };
  uint32_t part = P_HDR0;
  uint64_t val = strobe_begin_op(L, STROBE_M | STROBE_A);          // the part's bytes when it is a header or the length
  uint64_t rem = 2, off = 0;                                       // bytes left in the part, bytes of it done
  bool force = false;                                              // begin_op's run_f is due
  for (;;) {
    // 1. consume up to the block boundary
    while (part != P_END && L.pos < STROBE_RATE && !force) {
      if (rem == 0) {                                              // the next part begins here, at a position below the boundary
        ++part;
        off = 0;
        if (part == P_LABEL) {
          rem = lab_len;
        } else if (part == P_LEN) {
          val = frame_len;
          rem = 4;
        } else if (part == P_HDR1) {
          val = strobe_begin_op(L, SQUEEZE ? (STROBE_I | STROBE_A | STROBE_C) : STROBE_A);
          rem = 2;
        } else if (part == P_DATA) {
          rem = data_len;
          force = SQUEEZE && L.pos != 0;
        }
        continue;
      }
      const uint32_t nb = strobe_step(L.pos, rem);
      if (part == P_DATA) {
        if constexpr (SQUEEZE) io.put(off, strobe_squeeze_step(L, nb), nb);
        else strobe_absorb_step(L, io.get(off), nb);
      } else {
        strobe_absorb_step(L, part == P_LABEL ? strobe_label_fetch(lab, (uint32_t)off) : val >> (8 * off), nb);
      }
      off += nb;
      rem -= nb;
    }
    // 2. the lanes that stand at the boundary (or owe begin_op's run_f) permute, here and nowhere else
    if (L.pos == STROBE_RATE || force) {
      strobe_run_f(L);
      force = false;
    }
    // 3. repeat while input is left
    if (part == P_END) break;
  }
}

template <class Msg>
ZKP_HD void strobe_append_message(strobe_lane& L, const uint64_t* lab, uint32_t lab_len, const Msg& msg, uint64_t len) {
  strobe_merlin_op<false>(L, lab, lab_len, (uint32_t)len, len, msg);
}
template <class Out>
ZKP_HD void strobe_challenge_bytes(strobe_lane& L, const uint64_t* lab, uint32_t lab_len, const Out& out, uint32_t len) {
  strobe_merlin_op<true>(L, lab, lab_len, len, len, out);
}

// The position word pos | pos_begin << 8 | cur_flags << 16 after one append_message(label, msg) on a transcript whose position word is
// strobe_pos, by arithmetic alone: 2 + label_len + 4 + 2 + msg_len bytes are absorbed and nothing forces a permutation, so the position
// advances mod 166; ad's begin_op sets pos_begin behind its header's first byte and a later block boundary clears it.  A position byte
// >= 166 (a corrupt blob, which the calls pass through) returns strobe_pos unchanged.
ZKP_HD uint32_t strobe_pos_after_append(uint32_t strobe_pos, uint64_t label_len, uint64_t msg_len) {
  const uint32_t pos = strobe_pos & 0xffu;
  if (pos >= STROBE_RATE) return strobe_pos;
  const uint32_t at_ad = (uint32_t)((pos + 6 + label_len % STROBE_RATE) % STROBE_RATE);     // where ad's header begins
  const uint64_t m = msg_len % STROBE_RATE;
  const bool crossed = msg_len >= STROBE_RATE || at_ad + 2 + m >= STROBE_RATE;
  const uint32_t end = (uint32_t)((at_ad + 2 + m) % STROBE_RATE);
  return end | (crossed ? 0u : at_ad + 1) << 8 | STROBE_A << 16;
}

// ---- the part walker -------------------------------------------------------------------------------------------------------------------
// A part is a run of bytes that one STROBE duplex call moves.  SP_HDR is begin_op: its two header bytes are made when the part begins
// (they hold pos_begin), and a header whose flags carry C owes a run_f once it is absorbed if pos != 0 (Strobe128::begin_op) -- PRF's
// and KEY's alike.  SP_PRF64 is prf(64) whose output is reduced mod l: the C flag leaves it at pos = 0, so its 64 bytes are state words
// 0..7, read with constant indices (no byte loop, no run-time register index).
enum : uint32_t { SP_NONE, SP_HDR, SP_VAL, SP_LABEL, SP_AD, SP_KEY, SP_PRF, SP_PRF64, SP_END };
struct strobe_part {
  uint32_t kind, flags;         // flags: SP_HDR's operation flags
  uint64_t rem, val;            // bytes left; SP_VAL's bytes (little-endian, at most 8), SP_PRF64's output index, SP_LABEL's label number
  uint64_t len;                 // SP_AD / SP_KEY: the length of the whole message (strobe_msg's bound)
  const uint8_t* src;           // SP_AD / SP_KEY: the message
  uint8_t* dst;                 // SP_PRF: the output
};
ZKP_HD strobe_part strobe_part_make(uint32_t kind, uint32_t flags, uint64_t rem, uint64_t val, const uint8_t* src, uint8_t* dst) {
  strobe_part p;
  p.kind = kind; p.flags = flags; p.rem = rem; p.val = val; p.len = rem; p.src = src; p.dst = dst;
  return p;
}
ZKP_HD strobe_part strobe_part_hdr(uint32_t flags) { return strobe_part_make(SP_HDR, flags, 2, 0, nullptr, nullptr); }
ZKP_HD strobe_part strobe_part_val(uint64_t val, uint32_t n) { return strobe_part_make(SP_VAL, 0, n, val, nullptr, nullptr); }
ZKP_HD strobe_part strobe_part_label(uint32_t which, uint32_t n) { return strobe_part_make(SP_LABEL, 0, n, which, nullptr, nullptr); }
ZKP_HD strobe_part strobe_part_end() { return strobe_part_make(SP_END, 0, 0, 0, nullptr, nullptr); }

// Strobe128::overwrite of the low nb bytes of x, nb = strobe_step(pos, ..)
ZKP_HD void strobe_overwrite_step(strobe_lane& L, uint64_t x, uint32_t nb) {
  const uint32_t b = 8 * (L.pos & 7);
  const uint64_t m = tr_bytemask(nb), w = L.S[(L.pos >> 3) * L.stride];
  L.S[(L.pos >> 3) * L.stride] = (w & ~(m << b)) | (x & m) << b;
  L.pos += nb;
}

// Walks seq.part(0), seq.part(1), .. up to its SP_END on a valid lane, in strobe_merlin_op's loop: consume up to the block boundary;
// run_f at ONE place; repeat.  seq.label(k) = the words of label k (a pointer of the sequence's own: on the device it stays an LDS
// pointer, a part carries no pointer that could be either LDS or global); seq.wide(k, w) receives the eight state words of the k-th SP_PRF64.
template <class Seq>
ZKP_HD void strobe_walk(strobe_lane& L, Seq& seq) {
  strobe_part p = strobe_part_make(SP_NONE, 0, 0, 0, nullptr, nullptr);
  uint32_t idx = 0;
  uint64_t off = 0;
  bool force = false, owes = false;                                // begin_op's run_f is due / a header with the C flag is being absorbed
  for (;;) {
    // 1. consume up to the block boundary
    while (p.kind != SP_END && L.pos < STROBE_RATE && !force) {
      if (p.rem == 0) {
        if (owes) {                                                // the header is in, at a position below the boundary
          owes = false;
          force = L.pos != 0;
          continue;
        }
        p = seq.part(idx++);
        off = 0;
        if (p.kind == SP_HDR) {
          p.val = strobe_begin_op(L, p.flags);
          p.rem = 2;
          owes = (p.flags & STROBE_C) != 0;
        }
        continue;
      }
      if (p.kind == SP_PRF64) {                                    // pos = 0 here (see above)
        uint64_t w[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          w[i] = L.S[i * L.stride];
          L.S[i * L.stride] = 0;
        }
        L.pos = 64;
        seq.wide((uint32_t)p.val, w);
        p.rem = 0;
        continue;
      }
      const uint32_t nb = strobe_step(L.pos, p.rem);
      if (p.kind == SP_PRF) strobe_out{p.dst}.put(off, strobe_squeeze_step(L, nb), nb);
      else if (p.kind == SP_AD) strobe_absorb_step(L, strobe_msg{p.src, p.len}.get(off), nb);
      else if (p.kind == SP_KEY) strobe_overwrite_step(L, strobe_msg{p.src, p.len}.get(off), nb);
      else if (p.kind == SP_LABEL) strobe_absorb_step(L, strobe_label_fetch(seq.label((uint32_t)p.val), (uint32_t)off), nb);
      else strobe_absorb_step(L, p.val >> (8 * off), nb);         // SP_HDR, SP_VAL
      off += nb;
      p.rem -= nb;
    }
    // 2. the lanes that stand at the boundary (or owe begin_op's run_f) permute, here and nowhere else
    if (L.pos == STROBE_RATE || force) {
      strobe_run_f(L);
      force = false;
    }
    // 3. repeat while parts are left
    if (p.kind == SP_END) break;
  }
}

// from_bytes_mod_order_wide of the 64 bytes in w[0..8) -> 32 canonical bytes at out (any alignment)
ZKP_HD void strobe_wide_to_scalar(const uint64_t w[8], uint8_t* out) {
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    x[2 * i] = (uint32_t)w[i];
    x[2 * i + 1] = (uint32_t)(w[i] >> 32);
  }
  sc r;
  sc_reduce_wide(r, x);
  const strobe_out o{out};
#pragma unroll
  for (int i = 0; i < 4; ++i) o.put(8 * i, r.v[2 * i] | (uint64_t)r.v[2 * i + 1] << 32, 8);
}

// TranscriptRng on a clone of the transcript in L (Transcript::build_rng):
//   for k < m:  meta_ad(label); meta_ad(u32le(wlen), more); KEY(witness k)        -- rekey_with_witness_bytes(label, w_k)
//   meta_ad("rng"); KEY(entropy[32])                                              -- finalize
//   scalars:  count x { meta_ad(u32le(64)); PRF(64) -> mod l }  -> out [count][32]    -- Scalar::random
//   bytes:    meta_ad(u32le(count)); PRF(count)                 -> out [count]        -- fill_bytes
constexpr uint32_t STROBE_RNG_SCALARS = 0, STROBE_RNG_BYTES = 1;
template <uint32_t MODE>
struct strobe_rng_seq {
  const uint64_t* lab;
  uint32_t lab_len, m, wlen, count;
  const uint8_t* wit;          // [m][wlen]
  const uint8_t* entropy;      // [32]
  uint8_t* out;
  uint32_t g = 0, r = 0;       // the walk's place: frame g (witness g < m, finalize g = m, then the outputs), slot r of its five
  // Every frame has the same five slots -- header of meta_ad, label, u32le(length), header of the operation, data -- of which finalize has
  // no length and an output no label: an empty slot is a part of 0 bytes.  (The walker asks for the parts in order; its index is not used.)
  ZKP_HD strobe_part part(uint32_t) {
    const uint32_t rounds = MODE == STROBE_RNG_SCALARS ? count : 1u, fg = g, fr = r;
    if (fg > m + rounds) return strobe_part_end();
    r = fr == 4 ? 0 : fr + 1;
    g = fg + (fr == 4);
    const bool keyed = fg <= m, fin = fg == m;
    if (fr == 0) return strobe_part_hdr(STROBE_M | STROBE_A);
    if (fr == 1) return fg < m ? strobe_part_label(0, lab_len) : strobe_part_val(0x676e72u /* "rng" */, fin ? 3 : 0);
    if (fr == 2) return strobe_part_val(fg < m ? wlen : MODE == STROBE_RNG_SCALARS ? 64u : count, fin ? 0 : 4);
    if (fr == 3) return strobe_part_hdr(keyed ? STROBE_A | STROBE_C : STROBE_I | STROBE_A | STROBE_C);
    if (keyed) return strobe_part_make(SP_KEY, 0, fin ? 32u : wlen, 0, fin ? entropy : wit + (size_t)fg * wlen, nullptr);
    if (MODE == STROBE_RNG_SCALARS) return strobe_part_make(SP_PRF64, 0, 64, fg - m - 1, nullptr, nullptr);
    return strobe_part_make(SP_PRF, 0, count, 0, nullptr, out);
  }
  ZKP_HD const uint64_t* label(uint32_t) const { return lab; }
  ZKP_HD void wide(uint32_t k, const uint64_t w[8]) const { strobe_wide_to_scalar(w, out + 32 * (size_t)k); }
};

// TranscriptProtocol::get_challenge: challenge_bytes(label, 64) reduced mod l -> out[32]
struct strobe_challenge_scalar_seq {
  const uint64_t* lab;
  uint32_t lab_len;
  uint8_t* out;
  ZKP_HD strobe_part part(uint32_t i) const {
    if (i == 0) return strobe_part_hdr(STROBE_M | STROBE_A);
    if (i == 1) return strobe_part_label(0, lab_len);
    if (i == 2) return strobe_part_val(64, 4);
    if (i == 3) return strobe_part_hdr(STROBE_I | STROBE_A | STROBE_C);
    if (i == 4) return strobe_part_make(SP_PRF64, 0, 64, 0, nullptr, nullptr);
    return strobe_part_end();
  }
  ZKP_HD const uint64_t* label(uint32_t) const { return lab; }
  ZKP_HD void wide(uint32_t, const uint64_t w[8]) const { strobe_wide_to_scalar(w, out); }
};

// append_message(kind, var_label); append_message("val", point[32]) -- append_point_var ("ptvar") and append_blinding_commitment
// ("blindcom"); the validating forms return early on the identity's encoding, which is the caller's check (strobe_is_identity)
struct strobe_append_point_seq {
  const uint64_t* kind;
  const uint64_t* var;
  uint32_t kind_len, var_len;
  const uint8_t* point;
  ZKP_HD strobe_part part(uint32_t i) const {
    if (i == 0 || i == 5) return strobe_part_hdr(STROBE_M | STROBE_A);
    if (i == 1) return strobe_part_label(0, kind_len);
    if (i == 2) return strobe_part_val(var_len, 4);
    if (i == 3 || i == 8) return strobe_part_hdr(STROBE_A);
    if (i == 4) return strobe_part_label(1, var_len);
    if (i == 6) return strobe_part_val(0x6c6176u /* "val" */, 3);
    if (i == 7) return strobe_part_val(32, 4);
    if (i == 9) return strobe_part_make(SP_AD, 0, 32, 0, point, nullptr);
    return strobe_part_end();
  }
  ZKP_HD const uint64_t* label(uint32_t k) const { return k ? var : kind; }
  ZKP_HD void wide(uint32_t, const uint64_t*) const {}
};
// the 32 bytes at p (any alignment) are all zero: the encoding of the identity (public data: the reference branches on it too)
ZKP_HD bool strobe_is_identity(const uint8_t* p) {
  const strobe_msg m{p, 32};
  return (m.get(0) | m.get(8) | m.get(16) | m.get(24)) == 0;
}

}  // namespace zkp
