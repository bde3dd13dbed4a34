"""Batched Merlin operations without a GPU: zkp_amd/csrc/strobe_lane.h compiled by g++ against host Merlin in a stand-alone program under
AddressSanitizer and UBSan, zkp_strobe_pos_after_append against the host's blobs, and the toolbox's zkp_transcripts_append_message_batch_ctx /
zkp_transcripts_challenge_bytes_batch on their host route (ctx == NULL) against the call they extend, the single-transcript calls and
oracle/model.py's transcript.  Inputs: tests/transcript_ops_cases.py."""
import os
import random
import shutil
import subprocess

import numpy as np

from oracle import model as M
from tests.transcript_ops_cases import LABELS, LC, LM, RATE, append_sweep, host_append, host_challenge, message, pos_word, start_states
from zkp_amd import toolbox as T
from zkp_amd.engine import Engine, messages_csr, strobe_pos_after_append

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_BAD, T_TOO_LONG = -10, -14          # ZKP_TB_BAD_STATEMENT, ZKP_TB_TOO_LONG


def model_blob(t: M.Transcript) -> bytes:
    s = t.strobe
    return bytes(s.state) + bytes([s.pos, s.pos_begin, s.cur_flags]) + bytes(5)


def model_from_start(k: int) -> M.Transcript:
    t = M.Transcript(b"t")
    t.append_message(b"s", bytes((1 + (7 * i + k) % 255) for i in range(k)))
    return t


def append_ctx(ts, label, data, offsets, shared=False, threads=0, ctx=None):
    out = np.ascontiguousarray(ts).copy()
    n = len(offsets) - 1
    if shared:
        out = np.concatenate([out[:1], np.zeros((n - 1, 208), np.uint8)])
    rc = T.lib().zkp_transcripts_append_message_batch_ctx(ctx, T._p(out), n, int(shared), label, T._p(data), T._p(offsets), threads)
    assert rc == 0, rc
    return out


def test_start_states_cover_every_position():
    S = start_states()
    assert S.shape == (171, 208) and {int(b[200]) for b in S} == set(range(RATE))
    assert len({int(b[201]) for b in S}) == 2 and not S[:, 203:].any()      # pos_begin: ad's header, or 0 behind a block boundary
    assert len(LM) == 37 and len(LC) == 8 and [len(x) for x in LABELS] == [0, 3, 200]


def test_lane_code_equals_host_merlin_under_sanitizers(tmp_path):
    """tests/host/transcript_ops_host_main.cpp + host/merlin.cpp, g++ -fsanitize=address,undefined, as a child process: S x LM x labels through
    the lane code's append_message and S x LC x labels through its challenge_bytes, on heap blocks of exactly the message's and the
    output's size, each compared with Transcript over all 208 bytes (and every output byte); strobe_pos_after_append on every append."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (it builds the host library too)"
    exe = tmp_path / "transcript_ops_host_main"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "host", "transcript_ops_host_main.cpp"), os.path.join(ROOT, "zkp_amd", "csrc", "host", "merlin.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    n_app, n_chal = 3 * 171 * len(LM), 3 * 171 * len(LC)
    assert r.stdout.split("\n")[:-1] == ["append %d 0" % n_app, "challenge %d 0" % n_chal, "pos_after_append %d 0" % n_app, "positions 166"]


def test_pos_after_append_equals_the_host_blobs():
    ts, data, offsets = append_sweep()
    lens = np.diff(offsets.astype(np.int64))
    for label in LABELS:
        got = host_append(ts, label, data, offsets)
        for j in range(len(ts)):
            assert strobe_pos_after_append(pos_word(ts[j]), len(label), int(lens[j])) == pos_word(got[j]), (label[:4], j)
    assert Engine.strobe_pos_after_append(pos_word(ts[0]), 3, 32) == strobe_pos_after_append(pos_word(ts[0]), 3, 32)
    # long labels and messages: the arithmetic is mod 166, nothing overflows; a corrupt position word comes back as it is
    t = T.Transcript(b"t")
    before = pos_word(t.state)
    t.append_message(bytes(1000 * [97]), bytes(100000))
    assert strobe_pos_after_append(before, 1000, 100000) == pos_word(t.state)
    assert strobe_pos_after_append(200 | 7 << 8, 3, 32) == 200 | 7 << 8
    assert strobe_pos_after_append(3, 2**64 - 1, 2**64 - 1) & 0xff == (3 + 8 + 2 * ((2**64 - 1) % RATE)) % RATE


def test_new_append_with_no_context_gives_the_old_call_and_the_model():
    ts, data, offsets = append_sweep()
    rng = random.Random(5)
    for label in LABELS:
        want = host_append(ts, label, data, offsets)
        got = append_ctx(ts, label, data, offsets)
        assert (got == want).all()
        assert (T.append_messages_csr(ts.copy(), label, data, offsets, eng=None) == want).all()
        assert (T.append_messages_csr(ts.copy(), label, data, offsets, eng=T.HostEngine()) == want).all()
    # 64 sampled cases against the Python model and the single-transcript call
    for _ in range(64):
        s, li, label = rng.randrange(171), rng.randrange(len(LM)), rng.choice(LABELS)
        j = s * len(LM) + li
        msg = bytes(data[int(offsets[j]):int(offsets[j + 1])])
        assert len(msg) == LM[li]
        one = append_ctx(ts[j:j + 1], label, *messages_csr([msg]))
        m = model_from_start(s)
        assert model_blob(m) == ts[j].tobytes()
        m.append_message(label, msg)
        assert one[0].tobytes() == model_blob(m)
        t = T.Transcript(_state=ts[j])
        t.append_message(label, msg)
        assert (t.state == one[0]).all()
    # shared_initial: every transcript from row 0
    sh = append_ctx(ts, b"msg", data, offsets, shared=True)
    assert (sh == host_append(ts, b"msg", data, offsets, shared=True)).all()
    assert (sh == host_append(np.repeat(ts[:1], len(ts), axis=0), b"msg", data, offsets)).all()
    # a batch that does not start at offset 0 of the buffer
    assert (append_ctx(ts[100:300], b"msg", data, offsets[100:301]) == host_append(ts, b"msg", data, offsets)[100:300]).all()


def test_challenge_bytes_batch_equals_the_single_call_and_the_model():
    S = start_states()
    rng = random.Random(6)
    for label in LABELS:
        for n in LC:
            out, adv = host_challenge(S, label, n)
            assert (T.challenge_bytes(None, S.copy(), label, n) == out).all()
            for s in rng.sample(range(171), 3):
                t = T.Transcript(_state=S[s])
                assert t.challenge_bytes(label, n) == out[s].tobytes() and (t.state == adv[s]).all()
            s = rng.randrange(171)
            m = model_from_start(s)
            assert m.challenge_bytes(label, n) == out[s].tobytes() and model_blob(m) == adv[s].tobytes(), (label[:4], n, s)
    # len = 0 still advances the transcript (the frame, and the PRF's begin runs the permutation)
    out, adv = host_challenge(S, b"msg", 0)
    assert out.shape == (171, 0) and (adv != S).any(axis=1).all() and not adv[:, 200].any()


def test_one_and_sixteen_threads_give_the_same_bytes():
    ts, data, offsets = append_sweep()
    assert (append_ctx(ts, b"msg", data, offsets, threads=1) == append_ctx(ts, b"msg", data, offsets, threads=16)).all()
    S = np.repeat(start_states(), 4, axis=0)
    a, b = host_challenge(S, b"msg", 167, threads=1), host_challenge(S, b"msg", 167, threads=16)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


def test_no_ops_null_buffers_bad_offsets_and_bad_positions():
    lib, p = T.lib(), T._p
    S = start_states()[:4]
    data = np.arange(40, dtype=np.uint8)
    ok = np.array([0, 10, 10, 25, 40], np.uint64)
    dec = np.array([0, 10, 5, 25, 40], np.uint64)
    empty = np.zeros(5, np.uint64)
    out = np.zeros((4, 16), np.uint8)
    ts = S.copy()
    app, chal = lib.zkp_transcripts_append_message_batch_ctx, lib.zkp_transcripts_challenge_bytes_batch
    assert app(None, None, 0, 0, b"msg", None, None, 0) == 0 and chal(None, None, 0, b"msg", 16, 0, None) == 0
    assert app(None, None, 4, 0, b"msg", p(data), p(ok), 0) == T_BAD
    assert app(None, p(ts), 4, 0, b"msg", p(data), None, 0) == T_BAD
    assert app(None, p(ts), 4, 0, b"msg", None, p(ok), 0) == T_BAD
    assert app(None, p(ts), 4, 0, None, p(data), p(ok), 0) == T_BAD
    assert app(None, p(ts), 4, 0, b"msg", p(data), p(dec), 0) == T_BAD
    assert chal(None, None, 4, b"msg", 16, 0, p(out)) == T_BAD and chal(None, p(ts), 4, b"msg", 16, 0, None) == T_BAD
    assert chal(None, p(ts), 4, None, 16, 0, p(out)) == T_BAD
    # a position byte of 166 or more is no STROBE state: refused before any transcript changes (only row 0 counts when it is shared)
    bad = S.copy()
    bad[2, 200] = RATE
    assert app(None, p(bad), 4, 0, b"msg", p(data), p(ok), 0) == T_BAD and chal(None, p(bad), 4, b"msg", 16, 0, p(out)) == T_BAD
    assert (bad[[0, 1, 3]] == S[[0, 1, 3]]).all() and bad[2, 200] == RATE and (bad[2, :200] == S[2, :200]).all()
    assert (ts == S).all() and not out.any()
    assert app(None, p(bad), 4, 1, b"msg", p(data), p(ok), 0) == 0
    assert (bad == host_append(S, b"msg", data, ok, shared=True)).all()
    bad0 = S.copy()
    bad0[0, 200] = 255
    assert app(None, p(bad0), 4, 1, b"msg", p(data), p(ok), 0) == T_BAD
    # msgs may be NULL when every message is empty; len = 0 needs no output buffer
    assert app(None, p(ts), 4, 0, b"msg", None, p(empty), 0) == 0
    assert (ts == host_append(S, b"msg", data, empty)).all()
    ts = S.copy()
    assert chal(None, p(ts), 4, b"msg", 0, 0, None) == 0 and (ts == host_challenge(S, b"msg", 0)[1]).all()


def test_challenge_of_64_bytes_then_the_map_is_hash_to_group():
    S = np.repeat(start_states(), 2, axis=0)
    wide, adv = host_challenge(S, b"output", 64)
    ts = S.copy()
    want = T.hash_to_group(None, ts, b"output")
    assert (T.from_uniform_bytes(None, wide) == want).all() and (ts == adv).all()
