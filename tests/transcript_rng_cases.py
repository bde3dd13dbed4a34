"""Inputs shared by tests/test_host_transcript_rng.py and tests/test_gpu_transcript_rng.py: the witness shapes, counts and labels of the
batched witness RNG, challenge scalars and point appends (include/zkp_mi355x.h section 7), over the 171 start states of
tests/transcript_ops_cases.py (every position 0..165), and the host route they are compared with.

W       (m, wlen): no witness, an empty one, the ends of a state word, the reference's 32-byte scalars (1, 3 and 11 of them), one and two
        STROBE blocks of 166 bytes: KEY's forced permutation is met at pos = 0 and at pos != 0
COUNTS  scalars 1, 2, 5; bytes 0, 1, 64, around one block, and 400
LABELS  "", "w" and one of 200 bytes"""
import functools

import numpy as np

from tests.transcript_ops_cases import RATE, start_states  # noqa: F401  (re-exported)
from zkp_amd import toolbox as T

W = [(0, 0), (1, 0), (1, 1), (1, 32), (3, 32), (11, 32), (1, 165), (1, 166), (1, 167), (2, 333)]
SCALAR_COUNTS = [1, 2, 5]
BYTE_COUNTS = [0, 1, 64, 165, 166, 167, 400]
LABELS = [b"", b"w", bytes(ord("a") + i % 26 for i in range(200))]
KINDS = [b"ptvar", b"blindcom"]
EIGHT = [0, 1, 7, 8, 90, 163, 164, 165]       # positions: both ends of a state word and of the block, and one in the middle


def state_at(pos: int) -> int:
    """index of a start state that stands at position pos"""
    return int(np.flatnonzero(start_states()[:, 200] == pos)[0])


@functools.lru_cache(maxsize=None)
def _witnesses(n: int, m: int, wlen: int) -> bytes:
    return np.random.default_rng(1000 * m + wlen).integers(0, 256, size=(n, m, wlen), dtype=np.uint8).tobytes()


def witnesses(n: int, m: int, wlen: int) -> np.ndarray:
    """uint8 [n][m][wlen], the same for every caller"""
    return np.frombuffer(_witnesses(n, m, wlen), np.uint8).reshape(n, m, wlen).copy()


def entropy(n: int) -> np.ndarray:
    return np.random.default_rng(77).integers(0, 256, size=(n, 32), dtype=np.uint8)


def points(n: int, zero_rows=()) -> np.ndarray:
    """uint8 [n][32]: arbitrary non-zero rows (the appends validate nothing but the identity's encoding), zeros at zero_rows"""
    p = np.random.default_rng(78).integers(0, 256, size=(n, 32), dtype=np.uint8)
    p[:, 0] |= 1
    p[list(zero_rows)] = 0
    return p


@functools.lru_cache(maxsize=None)
def _host_rng(m: int, wlen: int, label: bytes, mode: int, count: int, n: int) -> bytes:
    f = T.witness_rng_scalars if mode == T.RNG_SCALARS else T.witness_rng_bytes
    return f(None, tiled_states(n), witnesses(n, m, wlen), count, entropy(n), label).tobytes()


def tiled_states(n: int) -> np.ndarray:
    """n blobs: the start states repeated in order"""
    S = start_states()
    return S if n == len(S) else np.ascontiguousarray(np.resize(S, (n, 208)))


def host_rng(m: int, wlen: int, label: bytes, mode: int, count: int, n: int = 171) -> np.ndarray:
    """the host route (eng = None) over tiled_states(n) with witnesses(n, m, wlen) and entropy(n); computed once per case"""
    out = np.frombuffer(_host_rng(m, wlen, label, mode, count, n), np.uint8)
    return out.reshape((n, count, 32) if mode == T.RNG_SCALARS else (n, count)).copy()
