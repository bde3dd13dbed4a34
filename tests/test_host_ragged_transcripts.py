"""Ragged transcript batches on the host: zkp_transcripts_append_message_batch (merlin append_message over a CSR batch) against the
oracle model and against per-call zkp_transcript_append_message, and the class grouping the _ragged device calls launch
(zkp_debug_ragged_blocks: pure host code of the test-hook library).  No GPU needed."""
import ctypes

import numpy as np
import pytest

from oracle import model as M
from zkp_amd import toolbox as T
from zkp_amd.engine import messages_csr, ragged_blocks

TB = T.TRANSCRIPT_BYTES


def model_blob(t: M.Transcript) -> bytes:
    s = t.strobe
    return bytes(s.state) + bytes([s.pos, s.pos_begin, s.cur_flags]) + bytes(5)


def _lengths():
    """0..600 with the rate boundaries (165/166/167) and two-block crossings"""
    return list(range(0, 40)) + [120, 140, 150, 155, 160, 163, 164, 165, 166, 167, 168, 200, 300, 331, 332, 333, 334, 400, 497, 498, 499, 600]


def _per_call(states, label, msgs):
    out = states.copy()
    for j, m in enumerate(msgs):
        t = T.Transcript(_state=out[j])
        t.append_message(label, m)
        out[j] = t.state
    return out


@pytest.mark.parametrize("threads", [1, 16])
def test_append_batch_matches_model_and_per_call(threads):
    rng = np.random.default_rng(3 + threads)
    lens = _lengths()
    msgs = [rng.bytes(n) for n in lens]
    # per-proof initial states, themselves at different positions
    init = []
    models = []
    for j in range(len(msgs)):
        m = M.Transcript(b"sig")
        m.append_message(b"pre", b"p" * (j % 170))
        models.append(m)
        init.append(np.frombuffer(model_blob(m), np.uint8))
    ts = np.stack(init).copy()
    want_calls = _per_call(ts, b"msg", msgs)
    got = T.append_messages(ts, b"msg", msgs, threads=threads)
    assert got is ts
    for j, m in enumerate(models):
        m.append_message(b"msg", msgs[j])
        assert bytes(ts[j]) == model_blob(m), j
    assert (ts == want_calls).all()


@pytest.mark.parametrize("threads", [1, 16])
def test_append_batch_shared_initial_state(threads):
    rng = np.random.default_rng(11)
    msgs = [rng.bytes(n) for n in _lengths()]
    got = T.append_messages(b"example signature", b"msg", msgs, threads=threads)
    for j, msg in enumerate(msgs):
        m = M.Transcript(b"example signature")
        m.append_message(b"msg", msg)
        assert bytes(got[j]) == model_blob(m)
    # the CSR form, with messages at arbitrary byte offsets inside a longer buffer
    data, off = messages_csr(msgs)
    pad = np.concatenate([np.zeros(7, np.uint8), data, np.zeros(3, np.uint8)])
    got2 = T.append_messages_csr(b"example signature", b"msg", pad, off + np.uint64(7), threads=threads)
    assert (got2 == got).all()


def test_append_batch_edges():
    lib = T.lib()
    # an empty batch: nothing to do, NULL buffers allowed
    assert lib.zkp_transcripts_append_message_batch(None, 0, 0, b"m", None, None, 1) == 0
    assert T.append_messages(b"x", b"m", []).shape == (0, TB)
    ts = np.stack([T.Transcript(b"t").state] * 3)
    before = ts.copy()
    off = np.array([0, 1, 2, 3], np.uint64)
    data = np.frombuffer(b"abc", np.uint8).copy()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    # NULL arguments
    assert lib.zkp_transcripts_append_message_batch(None, 3, 0, b"m", p(data), p(off), 1) == -10
    assert lib.zkp_transcripts_append_message_batch(p(ts), 3, 0, None, p(data), p(off), 1) == -10
    assert lib.zkp_transcripts_append_message_batch(p(ts), 3, 0, b"m", None, p(off), 1) == -10
    assert lib.zkp_transcripts_append_message_batch(p(ts), 3, 0, b"m", p(data), None, 1) == -10
    # decreasing offsets
    bad = np.array([0, 2, 1, 3], np.uint64)
    assert lib.zkp_transcripts_append_message_batch(p(ts), 3, 0, b"m", p(data), p(bad), 1) == -10
    # a message longer than merlin's u32 length prefix: ZKP_TB_TOO_LONG, decided from the offsets before any byte is read
    huge = np.array([0, 1, 2, 2 + (1 << 32)], np.uint64)
    assert lib.zkp_transcripts_append_message_batch(p(ts), 3, 0, b"m", p(data), p(huge), 1) == -14
    assert (ts == before).all()
    with pytest.raises(ValueError):
        T.append_messages_csr(ts, b"m", data, np.array([0, 1, 2], np.uint64))       # N from the offsets must match the array


def test_append_batch_empty_messages_and_null_data():
    """zero-length messages with no data buffer at all append the label and length prefix only"""
    lib = T.lib()
    ts = np.stack([T.Transcript(b"t").state] * 4)
    off = np.zeros(5, np.uint64)
    assert lib.zkp_transcripts_append_message_batch(ts.ctypes.data_as(ctypes.c_void_p), 4, 0, b"m", None, off.ctypes.data_as(ctypes.c_void_p), 1) == 0
    m = M.Transcript(b"t")
    m.append_message(b"m", b"")
    assert all(bytes(r) == model_blob(m) for r in ts)


def _ragged_states(lens, label=b"sig"):
    return T.append_messages(label, b"msg", [b"\x01" * n for n in lens])


@pytest.mark.parametrize("seed", [0, 1])
def test_class_grouping_and_block_table(seed):
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in rng.integers(0, 400, size=1000)] + [5] * 70       # a class of 70+ proofs spans several blocks
    ts = _ragged_states(lens)
    idx, blocks = ragged_blocks(ts)
    assert sorted(idx.tolist()) == list(range(len(lens)))                      # every proof exactly once
    pos = [bytes(ts[j, 200:203]) for j in range(len(lens))]
    order = []
    for p_ in pos:
        if p_ not in order:
            order.append(p_)                                                   # classes in order of first appearance
    want = [j for c in order for j in range(len(lens)) if pos[j] == c]          # stable within a class
    assert idx.tolist() == want
    covered = 0
    for cls, first, count in blocks.tolist():
        assert 1 <= count <= 32 and first == covered
        assert all(pos[idx[q]] == order[cls] for q in range(first, first + count))   # one class per block
        covered += count
    assert covered == len(lens)
    n_cls = [pos.count(c) for c in order]
    assert len(blocks) == sum((k + 31) // 32 for k in n_cls)


def test_class_grouping_aligned_and_single():
    ts = _ragged_states([7] * 65)
    idx, blocks = ragged_blocks(ts)
    assert idx.tolist() == list(range(65)) and blocks.tolist() == [[0, 0, 32], [0, 32, 32], [0, 64, 1]]
    idx, blocks = ragged_blocks(ts[:1])
    assert idx.tolist() == [0] and blocks.tolist() == [[0, 0, 1]]
