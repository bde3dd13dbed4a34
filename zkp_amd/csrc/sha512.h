// SHA-512 (FIPS 180-4) of byte ranges of one shared buffer, for the host and the device: the first half of curve25519-dalek's
// `RistrettoPoint::hash_from_bytes::<Sha512>` (reference tests/zkp.rs:34; the second half is ristretto_from_uniform_words of ge25519.h).
//
// g++ (host backend, and a stand-alone driver that includes nothing but this header) and hipcc compile the same text.  On the GPU the
// 64-bit words live in 32-bit halves, as in merlin_prog.h: a rotation is two v_alignbit_b32, the XOR of three values and Ch / Maj are
// one v_bitop3_b32 per half.  On the host the words are plain uint64_t.
//
// Branches and addresses depend on message LENGTHS only, never on message bytes: lengths are public in every use the reference makes.
// A message is a range [lo, hi) of a buffer of msgs_len bytes.  sha512_clamp cuts the range to [0, msgs_len) first, whatever lo and hi
// hold (hi < lo is empty): a bad range gives a wrong digest, never a read outside the buffer.
#pragma once
#include <stdint.h>

#ifndef ZKP_HD
#if defined(__HIPCC__)
#define ZKP_HD __host__ __device__ __forceinline__
#else
#define ZKP_HD inline
#endif
#endif

namespace zkp {

// The range [lo, hi) clamped to [0, msgs_len): lo is cut to msgs_len, hi too, and hi < lo reads as empty.  Updates lo, returns the length.
ZKP_HD uint64_t sha512_clamp(uint64_t& lo, uint64_t hi, uint64_t msgs_len) {
  lo = lo < msgs_len ? lo : msgs_len;
  hi = hi < msgs_len ? hi : msgs_len;
  return hi > lo ? hi - lo : 0;
}

// rotation right by a compile-time amount, 0 < N < 64
template <int N>
ZKP_HD uint64_t sha512_rotr(uint64_t v) {
#ifdef __HIP_DEVICE_COMPILE__
  constexpr int n = N & 31;
  const uint32_t a = (N & 32) ? (uint32_t)v : (uint32_t)(v >> 32);      // high and low half after the rotation by N & 32 (a swap)
  const uint32_t b = (N & 32) ? (uint32_t)(v >> 32) : (uint32_t)v;
  if (n == 0) return (uint64_t)a << 32 | b;
  return (uint64_t)__builtin_amdgcn_alignbit(b, a, n) << 32 | __builtin_amdgcn_alignbit(a, b, n);
#else
  return (v >> N) | (v << (64 - N));
#endif
}
// shift right by a compile-time amount, 0 < N < 32
template <int N>
ZKP_HD uint64_t sha512_shr(uint64_t v) {
#ifdef __HIP_DEVICE_COMPILE__
  const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  return (uint64_t)(hi >> N) << 32 | __builtin_amdgcn_alignbit(hi, lo, N);
#else
  return v >> N;
#endif
}

// one v_bitop3_b32 per half with truth table T over (a, b, c) = (0xF0, 0xCC, 0xAA)
template <int T>
ZKP_HD uint64_t sha512_bitop3(uint64_t a, uint64_t b, uint64_t c) {
#ifdef __HIP_DEVICE_COMPILE__
  return (uint64_t)(uint32_t)__builtin_amdgcn_bitop3_b32((uint32_t)(a >> 32), (uint32_t)(b >> 32), (uint32_t)(c >> 32), T) << 32 |
         (uint32_t)__builtin_amdgcn_bitop3_b32((uint32_t)a, (uint32_t)b, (uint32_t)c, T);
#else
  uint64_t r = 0;
  if (T & 0x80) r |= a & b & c;
  if (T & 0x40) r |= a & b & ~c;
  if (T & 0x20) r |= a & ~b & c;
  if (T & 0x10) r |= a & ~b & ~c;
  if (T & 0x08) r |= ~a & b & c;
  if (T & 0x04) r |= ~a & b & ~c;
  if (T & 0x02) r |= ~a & ~b & c;
  if (T & 0x01) r |= ~a & ~b & ~c;
  return r;
#endif
}
ZKP_HD uint64_t sha512_xor3(uint64_t a, uint64_t b, uint64_t c) { return sha512_bitop3<0x96>(a, b, c); }
ZKP_HD uint64_t sha512_ch(uint64_t e, uint64_t f, uint64_t g) { return sha512_bitop3<0xCA>(e, f, g); }     // e ? f : g
ZKP_HD uint64_t sha512_maj(uint64_t a, uint64_t b, uint64_t c) { return sha512_bitop3<0xE8>(a, b, c); }   // majority

ZKP_HD void sha512_init(uint64_t H[8]) {
  H[0] = 0x6a09e667f3bcc908ULL; H[1] = 0xbb67ae8584caa73bULL; H[2] = 0x3c6ef372fe94f82bULL; H[3] = 0xa54ff53a5f1d36f1ULL;
  H[4] = 0x510e527fade682d1ULL; H[5] = 0x9b05688c2b3e6c1fULL; H[6] = 0x1f83d9abfb41bd6bULL; H[7] = 0x5be0cd19137e2179ULL;
}

// One compression (FIPS 180-4 section 6.4.2) of the block W[16] (big-endian words; overwritten by the message schedule) into H.
// The 80 rounds are unrolled so that W stays in registers and every K[t] is an immediate.
ZKP_HD void sha512_compress(uint64_t H[8], uint64_t W[16]) {
  const uint64_t K[80] = {
      0x428a2f98d728ae22ULL, 0x7137449123ef65cdULL, 0xb5c0fbcfec4d3b2fULL, 0xe9b5dba58189dbbcULL,
      0x3956c25bf348b538ULL, 0x59f111f1b605d019ULL, 0x923f82a4af194f9bULL, 0xab1c5ed5da6d8118ULL,
      0xd807aa98a3030242ULL, 0x12835b0145706fbeULL, 0x243185be4ee4b28cULL, 0x550c7dc3d5ffb4e2ULL,
      0x72be5d74f27b896fULL, 0x80deb1fe3b1696b1ULL, 0x9bdc06a725c71235ULL, 0xc19bf174cf692694ULL,
      0xe49b69c19ef14ad2ULL, 0xefbe4786384f25e3ULL, 0x0fc19dc68b8cd5b5ULL, 0x240ca1cc77ac9c65ULL,
      0x2de92c6f592b0275ULL, 0x4a7484aa6ea6e483ULL, 0x5cb0a9dcbd41fbd4ULL, 0x76f988da831153b5ULL,
      0x983e5152ee66dfabULL, 0xa831c66d2db43210ULL, 0xb00327c898fb213fULL, 0xbf597fc7beef0ee4ULL,
      0xc6e00bf33da88fc2ULL, 0xd5a79147930aa725ULL, 0x06ca6351e003826fULL, 0x142929670a0e6e70ULL,
      0x27b70a8546d22ffcULL, 0x2e1b21385c26c926ULL, 0x4d2c6dfc5ac42aedULL, 0x53380d139d95b3dfULL,
      0x650a73548baf63deULL, 0x766a0abb3c77b2a8ULL, 0x81c2c92e47edaee6ULL, 0x92722c851482353bULL,
      0xa2bfe8a14cf10364ULL, 0xa81a664bbc423001ULL, 0xc24b8b70d0f89791ULL, 0xc76c51a30654be30ULL,
      0xd192e819d6ef5218ULL, 0xd69906245565a910ULL, 0xf40e35855771202aULL, 0x106aa07032bbd1b8ULL,
      0x19a4c116b8d2d0c8ULL, 0x1e376c085141ab53ULL, 0x2748774cdf8eeb99ULL, 0x34b0bcb5e19b48a8ULL,
      0x391c0cb3c5c95a63ULL, 0x4ed8aa4ae3418acbULL, 0x5b9cca4f7763e373ULL, 0x682e6ff3d6b2b8a3ULL,
      0x748f82ee5defb2fcULL, 0x78a5636f43172f60ULL, 0x84c87814a1f0ab72ULL, 0x8cc702081a6439ecULL,
      0x90befffa23631e28ULL, 0xa4506cebde82bde9ULL, 0xbef9a3f7b2c67915ULL, 0xc67178f2e372532bULL,
      0xca273eceea26619cULL, 0xd186b8c721c0c207ULL, 0xeada7dd6cde0eb1eULL, 0xf57d4f7fee6ed178ULL,
      0x06f067aa72176fbaULL, 0x0a637dc5a2c898a6ULL, 0x113f9804bef90daeULL, 0x1b710b35131c471bULL,
      0x28db77f523047d84ULL, 0x32caab7b40c72493ULL, 0x3c9ebe0a15c9bebcULL, 0x431d67c49c100d4cULL,
      0x4cc5d4becb3e42b6ULL, 0x597f299cfc657e2aULL, 0x5fcb6fab3ad6faecULL, 0x6c44198c4a475817ULL,
  };
  uint64_t a = H[0], b = H[1], c = H[2], d = H[3], e = H[4], f = H[5], g = H[6], h = H[7];
#pragma unroll
  for (int t = 0; t < 80; ++t) {
    uint64_t w = W[t & 15];
    if (t >= 16) {
      const uint64_t w1 = W[(t - 2) & 15], w15 = W[(t - 15) & 15];
      w += sha512_xor3(sha512_rotr<19>(w1), sha512_rotr<61>(w1), sha512_shr<6>(w1)) + W[(t - 7) & 15] +
           sha512_xor3(sha512_rotr<1>(w15), sha512_rotr<8>(w15), sha512_shr<7>(w15));
      W[t & 15] = w;
    }
    const uint64_t t1 = h + sha512_xor3(sha512_rotr<14>(e), sha512_rotr<18>(e), sha512_rotr<41>(e)) + sha512_ch(e, f, g) + K[t] + w;
    const uint64_t t2 = sha512_xor3(sha512_rotr<28>(a), sha512_rotr<34>(a), sha512_rotr<39>(a)) + sha512_maj(a, b, c);
    h = g; g = f; f = e; e = d + t1;
    d = c; c = b; b = a; a = t1 + t2;
  }
  H[0] += a; H[1] += b; H[2] += c; H[3] += d; H[4] += e; H[5] += f; H[6] += g; H[7] += h;
}

// Padding (FIPS 180-4 section 5.1.2) of the 8 message bytes at p (a multiple of 8), given little-endian in le: the bytes at or past
// len are cleared (whatever le held there) and the 0x80 byte goes to position len.  Returns the big-endian schedule word.  The length
// field is added by the caller.
ZKP_HD uint64_t sha512_pad_word(uint64_t le, uint64_t len, uint64_t p) {
  const uint64_t r = len > p ? len - p : 0;                                  // message bytes in this word (8 or more: all)
  const uint64_t keep = r >= 8 ? ~0ULL : (1ULL << (8 * r)) - 1;
  const uint64_t pad = (len >= p && len - p < 8) ? 0x80ULL << (8 * (len - p)) : 0;
  return __builtin_bswap64((le & keep) | pad);
}

// SHA-512 of the message msgs[lo, hi), clamped to [0, msgs_len) first.  H = the state after the last block (sha512_digest_words turns
// it into the digest).  Loops over ceil((len + 17) / 128) blocks: the length decides the branches, the bytes never do.
//   host:   byte loads, each of a byte of the message.
//   device: aligned dword loads funnel-shifted by the start's byte offset.  Dword k (from the one holding the first message byte) is
//           loaded only if it holds a byte of the message, so no load reaches an aligned dword that lies outside the buffer: no read can
//           cross into another page or allocation.  The bytes of a loaded dword that lie outside the message are cleared by the padding.
ZKP_HD void sha512_range(uint64_t H[8], const uint8_t* msgs, uint64_t msgs_len, uint64_t lo, uint64_t hi) {
  const uint64_t len = sha512_clamp(lo, hi, msgs_len);
  const uint8_t* m = msgs + lo;
  const uint64_t nblocks = (len + 17 + 127) >> 7;                           // message, the 0x80 byte, the 16-byte length
  sha512_init(H);
#ifdef __HIP_DEVICE_COMPILE__
  const uint32_t sh = (uint32_t)((uintptr_t)m & 3);
  const uint32_t* d = reinterpret_cast<const uint32_t*>(m - sh);
  const uint64_t span = len ? sh + len : 0;                                 // dword k holds a message byte iff 4 k < span
  uint32_t carry = span ? d[0] : 0u;                                        // dword 2 p / 8 of the next word
#endif
#pragma unroll 1
  for (uint64_t blk = 0; blk < nblocks; ++blk) {
    uint64_t W[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint64_t p = 128 * blk + 8 * (uint64_t)j;
#ifdef __HIP_DEVICE_COMPILE__
      const uint64_t q = p >> 2;
      const uint32_t d1 = 4 * (q + 1) < span ? d[q + 1] : 0u;
      const uint32_t d2 = 4 * (q + 2) < span ? d[q + 2] : 0u;
      const uint64_t le = (uint64_t)__builtin_amdgcn_alignbit(d2, d1, 8 * sh) << 32 | __builtin_amdgcn_alignbit(d1, carry, 8 * sh);
      carry = d2;
#else
      uint64_t le = 0;
      for (int k = 0; k < 8; ++k)
        if (p + k < len) le |= (uint64_t)m[p + k] << (8 * k);
#endif
      W[j] = sha512_pad_word(le, len, p);
    }
    const bool last = blk + 1 == nblocks;                                   // the message length in bits, as 128 bits big-endian
    W[14] |= last ? len >> 61 : 0;
    W[15] |= last ? len << 3 : 0;
    sha512_compress(H, W);
  }
}

// The 64-byte digest of the state H as 16 little-endian dwords (byte 4 i + k of the digest = byte k of w[i]).
ZKP_HD void sha512_digest_words(uint32_t w[16], const uint64_t H[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    w[2 * j] = __builtin_bswap32((uint32_t)(H[j] >> 32));
    w[2 * j + 1] = __builtin_bswap32((uint32_t)H[j]);
  }
}

}  // namespace zkp
