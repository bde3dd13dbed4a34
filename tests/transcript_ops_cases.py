"""Inputs shared by tests/test_host_transcript_ops.py and tests/test_gpu_transcript_ops.py: the start states, message lengths, challenge
lengths and labels of the batched Merlin operations (include/zkp_mi355x.h section 7), and the host route they are compared with.

S   171 blobs: Transcript("t") with k bytes appended under the label "s", k = 0..170: every pos 0..165 and a spread of pos_begin
LM  message lengths: around a state word, around one and two blocks of 166 bytes, and 600
LC  challenge lengths: 0, the common 32 and 64, around one block, and 400
LABELS  "", "msg" and one of 200 bytes, under which the two header bytes and the label itself cross a block"""
import functools

import numpy as np

from zkp_amd import toolbox as T

LM = [0, 1, 2, 7, 8, 9] + list(range(150, 176)) + [331, 332, 333, 334, 600]
LC = [0, 1, 32, 64, 165, 166, 167, 400]
LABELS = [b"", b"msg", bytes(ord("a") + i % 26 for i in range(200))]
RATE = 166


@functools.lru_cache(maxsize=None)
def _start_states() -> bytes:
    rows = []
    for k in range(171):
        t = T.Transcript(b"t")
        t.append_message(b"s", bytes((1 + (7 * i + k) % 255) for i in range(k)))
        rows.append(t.state.tobytes())
    return b"".join(rows)


def start_states() -> np.ndarray:
    """S as a fresh uint8 [171][208] array"""
    return np.frombuffer(_start_states(), np.uint8).reshape(171, 208).copy()


def pos_word(blob) -> int:
    return int(blob[200]) | int(blob[201]) << 8 | int(blob[202]) << 16


def message(length: int, salt: int) -> bytes:
    return bytes((31 * i + length + salt) & 0xff for i in range(length))


@functools.lru_cache(maxsize=None)
def _append_sweep():
    S = start_states()
    ts = np.repeat(S, len(LM), axis=0)                                     # row = start * len(LM) + length index
    msgs = [message(n, int(S[s][200])) for s in range(len(S)) for n in LM]
    from zkp_amd.engine import messages_csr
    data, offsets = messages_csr(msgs)
    return ts.tobytes(), data.tobytes(), offsets.tobytes()


def append_sweep():
    """S x LM as one CSR batch: (transcripts [171 * 37][208], data, offsets), fresh arrays"""
    ts, data, offsets = _append_sweep()
    return (np.frombuffer(ts, np.uint8).reshape(-1, 208).copy(), np.frombuffer(data, np.uint8).copy(), np.frombuffer(offsets, np.uint64).copy())


def host_append(ts, label: bytes, data, offsets, shared: bool = False, threads: int = 0) -> np.ndarray:
    """the parent route: zkp_transcripts_append_message_batch on a copy of ts"""
    out = np.ascontiguousarray(ts).copy()
    n = len(offsets) - 1
    if shared:
        out = np.concatenate([out[:1], np.zeros((n - 1, 208), np.uint8)]) if n else out[:0]
    rc = T.lib().zkp_transcripts_append_message_batch(T._p(out), n, int(shared), label, T._p(data), T._p(offsets), threads)
    assert rc == 0, rc
    return out


def host_challenge(ts, label: bytes, n_bytes: int, threads: int = 0):
    """the host route of zkp_transcripts_challenge_bytes_batch (ctx == NULL) on a copy of ts -> (out [N][n_bytes], advanced copy)"""
    adv = np.ascontiguousarray(ts).copy()
    out = np.zeros((len(adv), n_bytes), np.uint8)
    rc = T.lib().zkp_transcripts_challenge_bytes_batch(None, T._p(adv), len(adv), label, n_bytes, threads, T._p(out))
    assert rc == 0, rc
    return out, adv
