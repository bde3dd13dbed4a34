// Stand-alone driver of zkp_amd/csrc/strobe_lane.h on the host, built with g++ -fsanitize=address,undefined by
// tests/test_host_transcript_ops.py together with zkp_amd/csrc/host/merlin.cpp: the lane code's append_message and challenge_bytes
// against Transcript::append_message / challenge_bytes, over all 208 bytes of the blob and every output byte.
//
//   start states S:  Transcript("t") with k zero-free bytes appended under the label "s", k = 0..170: every pos 0..165 and a spread of pos_begin
//   message lengths Lm = {0, 1, 2, 7, 8, 9, 150..175, 331..334, 600};  challenge lengths Lc = {0, 1, 32, 64, 165, 166, 167, 400}
//   labels: "", "msg" and one of 200 bytes (the two header bytes and the label itself cross a block)
// Messages and outputs are heap blocks of exactly their length.  strobe_pos_after_append is compared with bytes 200..202 of every append.
//   stdout: "append <cases> <mismatches>", "challenge <cases> <mismatches>", "pos_after_append <cases> <mismatches>", "positions <distinct pos>"
//   exit status 1 on any mismatch
#include "../../zkp_amd/csrc/strobe_lane.h"
#include "../../zkp_amd/csrc/host/merlin.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

using zkp::host::Transcript;

static uint8_t* block(size_t bytes) { return bytes ? static_cast<uint8_t*>(malloc(bytes)) : nullptr; }

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
  std::vector<size_t> Lm = {0, 1, 2, 7, 8, 9, 331, 332, 333, 334, 600}, Lc = {0, 1, 32, 64, 165, 166, 167, 400};
  for (size_t n = 150; n <= 175; ++n) Lm.push_back(n);
  std::string long_label;
  for (int i = 0; i < 200; ++i) long_label.push_back((char)('a' + i % 26));
  const std::string labels[3] = {"", "msg", long_label};

  long n_app = 0, bad_app = 0, n_chal = 0, bad_chal = 0, n_pos = 0, bad_pos = 0;
  for (const std::string& label : labels) {
    zkp::strobe_label lab;
    if (!zkp::strobe_label_pack(lab, label.c_str(), label.size())) return 2;
    for (const auto& start : S) {
      for (size_t len : Lm) {
        uint8_t* msg = block(len);
        for (size_t i = 0; i < len; ++i) msg[i] = (uint8_t)(31 * i + len + start[200]);
        Transcript t = Transcript::from_bytes(start.data());
        t.append_message(label.c_str(), msg, len);
        uint8_t want[208];
        t.to_bytes(want);
        alignas(8) uint64_t in[26], out[26], col[25];
        memcpy(in, start.data(), 208);
        zkp::strobe_lane L{col, 1, 0, 0, 0};
        zkp::strobe_load(L, in);
        if (!zkp::strobe_valid(L)) return 2;
        zkp::strobe_append_message(L, lab.w, lab.len, zkp::strobe_msg{msg, len}, len);
        zkp::strobe_store(L, out, zkp::strobe_tail(L));
        ++n_app;
        if (memcmp(out, want, 208) != 0) ++bad_app;
        const uint32_t before = start[200] | start[201] << 8 | start[202] << 16, after = want[200] | want[201] << 8 | want[202] << 16;
        ++n_pos;
        if (zkp::strobe_pos_after_append(before, label.size(), len) != after) ++bad_pos;
        free(msg);
      }
      for (size_t len : Lc) {
        uint8_t* want_out = block(len);
        uint8_t* got_out = block(len);
        Transcript t = Transcript::from_bytes(start.data());
        t.challenge_bytes(label.c_str(), want_out, len);
        uint8_t want[208];
        t.to_bytes(want);
        alignas(8) uint64_t in[26], out[26], col[25];
        memcpy(in, start.data(), 208);
        zkp::strobe_lane L{col, 1, 0, 0, 0};
        zkp::strobe_load(L, in);
        zkp::strobe_challenge_bytes(L, lab.w, lab.len, zkp::strobe_out{got_out}, (uint32_t)len);
        zkp::strobe_store(L, out, zkp::strobe_tail(L));
        ++n_chal;
        if (memcmp(out, want, 208) != 0 || (len && memcmp(got_out, want_out, len) != 0)) ++bad_chal;
        free(want_out);
        free(got_out);
      }
    }
  }
  printf("append %ld %ld\nchallenge %ld %ld\npos_after_append %ld %ld\npositions %zu\n", n_app, bad_app, n_chal, bad_chal, n_pos, bad_pos, positions.size());
  return (bad_app || bad_chal || bad_pos) ? 1 : 0;
}
