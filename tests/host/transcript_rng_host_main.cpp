// Stand-alone driver of the part walker of zkp_amd/csrc/strobe_lane.h on the host, built with g++ -fsanitize=address,undefined by
// tests/test_host_transcript_rng.py together with zkp_amd/csrc/host/merlin.cpp: the lane code's witness RNG, get_challenge and point
// appends against host Merlin's Strobe128, TranscriptRng and Transcript, over all 208 bytes of the blob and every output byte.
//
//   start states S:  Transcript("t") with k zero-free bytes appended under the label "s", k = 0..170: every pos 0..165
//   witness shapes W (m, wlen): (0,0) (1,0) (1,1) (1,32) (3,32) (11,32) (1,165) (1,166) (1,167) (2,333)
//   counts: scalars 1, 2, 5; bytes 0, 1, 64, 165, 166, 167, 400;   labels: "", "w" and one of 200 bytes
// Witnesses, entropy, points and outputs are heap blocks of exactly their length (a read or write past one is the sanitizer's).
//   stdout: "rng_scalars <cases> <mismatches>", "rng_bytes ..", "challenge_scalars ..", "append_points ..", "validate ..",
//           "positions <distinct pos>";  exit status 1 on any mismatch
#include "../../zkp_amd/csrc/strobe_lane.h"
#include "../../zkp_amd/csrc/host/merlin.hpp"
#include "../../zkp_amd/csrc/host/scalar.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

using zkp::host::Scalar;
using zkp::host::Transcript;
using zkp::host::TranscriptRng;

static uint8_t* block(size_t bytes) { return bytes ? static_cast<uint8_t*>(malloc(bytes)) : nullptr; }

static void load(zkp::strobe_lane& L, const std::vector<uint8_t>& blob) {
  alignas(8) uint64_t in[26];
  memcpy(in, blob.data(), 208);
  zkp::strobe_load(L, in);
  if (!zkp::strobe_valid(L)) exit(2);
}
static void store(const zkp::strobe_lane& L, uint8_t out[208]) {
  alignas(8) uint64_t o[26];
  zkp::strobe_store(L, o, zkp::strobe_tail(L));
  memcpy(out, o, 208);
}

int main() {
  std::vector<std::vector<uint8_t>> S;
  std::set<int> positions;
  for (int k = 0; k <= 170; ++k) {
    Transcript t("t", 1);
    std::vector<uint8_t> m(k);
    for (int i = 0; i < k; ++i) m[i] = (uint8_t)(1 + (7 * i + k) % 255);
    t.append_message("s", m.data(), m.size());
    std::vector<uint8_t> blob(208);
    t.to_bytes(blob.data());
    positions.insert(blob[200]);
    S.push_back(blob);
  }
  const uint32_t W[10][2] = {{0, 0}, {1, 0}, {1, 1}, {1, 32}, {3, 32}, {11, 32}, {1, 165}, {1, 166}, {1, 167}, {2, 333}};
  const uint32_t CS[3] = {1, 2, 5}, CB[7] = {0, 1, 64, 165, 166, 167, 400};
  std::string long_label;
  for (int i = 0; i < 200; ++i) long_label.push_back((char)('a' + i % 26));
  const std::string labels[3] = {"", "w", long_label};

  long n_sc = 0, bad_sc = 0, n_by = 0, bad_by = 0, n_ch = 0, bad_ch = 0, n_ap = 0, bad_ap = 0, n_va = 0, bad_va = 0;
  for (const std::string& label : labels) {
    zkp::strobe_label lab;
    if (!zkp::strobe_label_pack(lab, label.c_str(), label.size())) return 2;
    for (size_t s = 0; s < S.size(); ++s) {
      const auto& start = S[s];
      for (const auto& shape : W) {
        const uint32_t m = shape[0], wlen = shape[1];
        uint8_t* wit = block((size_t)m * wlen);
        for (size_t i = 0; i < (size_t)m * wlen; ++i) wit[i] = (uint8_t)(29 * i + 3 * s + wlen + 1);
        uint8_t* ent = block(32);
        for (int i = 0; i < 32; ++i) ent[i] = (uint8_t)(211 * i + s + m);
        for (int mode = 0; mode < 2; ++mode) {
          for (int ci = 0; ci < (mode == 0 ? 3 : 7); ++ci) {
            const uint32_t count = mode == 0 ? CS[ci] : CB[ci];
            const size_t row = mode == 0 ? 32 * (size_t)count : count;
            uint8_t* want = block(row);
            uint8_t* got = block(row);
            TranscriptRng rng = Transcript::from_bytes(start.data()).build_rng();
            for (uint32_t k = 0; k < m; ++k) rng.rekey_with_witness_bytes(label.c_str(), wit + (size_t)k * wlen, wlen);
            rng.finalize(ent);
            if (mode == 0) {
              for (uint32_t k = 0; k < count; ++k) {
                uint8_t wide[64];
                rng.fill_bytes(wide, 64);
                Scalar::from_bytes_mod_order_wide(wide).to_bytes(want + 32 * k);
              }
            } else {
              rng.fill_bytes(want, count);
            }
            alignas(8) uint64_t col[25];
            zkp::strobe_lane L{col, 1, 0, 0, 0};
            load(L, start);
            if (mode == 0) {
              zkp::strobe_rng_seq<zkp::STROBE_RNG_SCALARS> seq{lab.w, lab.len, m, wlen, count, wit, ent, got};
              zkp::strobe_walk(L, seq);
            } else {
              zkp::strobe_rng_seq<zkp::STROBE_RNG_BYTES> seq{lab.w, lab.len, m, wlen, count, wit, ent, got};
              zkp::strobe_walk(L, seq);
            }
            const bool bad = row && memcmp(got, want, row) != 0;
            if (mode == 0) { ++n_sc; bad_sc += bad; } else { ++n_by; bad_by += bad; }
            free(want);
            free(got);
          }
        }
        free(wit);
        free(ent);
      }
      {                                                              // get_challenge
        uint8_t want_out[32], want[208], have[208];
        uint8_t* got_out = block(32);
        Transcript t = Transcript::from_bytes(start.data());
        t.get_challenge(label.c_str(), want_out);
        t.to_bytes(want);
        alignas(8) uint64_t col[25];
        zkp::strobe_lane L{col, 1, 0, 0, 0};
        load(L, start);
        zkp::strobe_challenge_scalar_seq seq{lab.w, lab.len, got_out};
        zkp::strobe_walk(L, seq);
        store(L, have);
        ++n_ch;
        if (memcmp(have, want, 208) != 0 || memcmp(got_out, want_out, 32) != 0) ++bad_ch;
        free(got_out);
      }
      for (const std::string& kind : {std::string("ptvar"), std::string("blindcom"), long_label}) {      // the appends: `label` names the variable
        zkp::strobe_label kl;
        if (!zkp::strobe_label_pack(kl, kind.c_str(), kind.size())) return 2;
        for (int zero = 0; zero < 2; ++zero) {
          uint8_t* pt = block(32);
          for (int i = 0; i < 32; ++i) pt[i] = zero ? 0 : (uint8_t)(17 * i + s + 1);
          uint8_t want[208], have[208];
          Transcript t = Transcript::from_bytes(start.data());
          t.append_message(kind.c_str(), label.data(), label.size());
          t.append_message("val", pt, 32);
          t.to_bytes(want);
          alignas(8) uint64_t col[25];
          zkp::strobe_lane L{col, 1, 0, 0, 0};
          load(L, start);
          zkp::strobe_append_point_seq seq{kl.w, lab.w, kl.len, lab.len, pt};
          zkp::strobe_walk(L, seq);
          store(L, have);
          ++n_ap;
          if (memcmp(have, want, 208) != 0) ++bad_ap;
          // the validating forms' test, against Transcript's own
          Transcript v = Transcript::from_bytes(start.data());
          const bool accepted = kind == "blindcom" ? v.validate_and_append_blinding_commitment(label.c_str(), pt) : v.validate_and_append_point_var(label.c_str(), pt);
          ++n_va;
          if (accepted == zkp::strobe_is_identity(pt)) ++bad_va;
          if (accepted && kind != long_label) {
            v.to_bytes(want);
            if (memcmp(have, want, 208) != 0) ++bad_va;
          }
          free(pt);
        }
      }
    }
  }
  printf("rng_scalars %ld %ld\nrng_bytes %ld %ld\nchallenge_scalars %ld %ld\nappend_points %ld %ld\nvalidate %ld %ld\npositions %zu\n",
         n_sc, bad_sc, n_by, bad_by, n_ch, bad_ch, n_ap, bad_ap, n_va, bad_va, positions.size());
  return (bad_sc || bad_by || bad_ch || bad_ap || bad_va) ? 1 : 0;
}
