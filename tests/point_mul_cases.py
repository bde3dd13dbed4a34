"""(helper module of tests/test_host_point_mul.py and tests/test_gpu_point_mul.py)
Operands of the batched Scalar * basepoint and Scalar * point calls, and their expected encodings from the oracle.

Scalars: the 148-value catalogue of tests/scalar_edge_cases.py (the edges of every recoder, the fold boundaries, multiples of l), the edges
0, 1, l - 1, l, l + 1, 2^255, 2^256 - 1, for each walk's window width w -- 4 (the radix-16 ladder of k_mul_pairs and the host backend) and
HOT_W = 7 (the fixed-base walk of k_mul_base) -- the 256-bit scalars whose every w-bit window equals 0, 1, 2^(w-1) - 1, 2^(w-1) and 2^w - 1,
and a seeded random sample.
Points: B, the identity (32 zero bytes), a few outputs of hash_from_bytes::<Sha512> (from the oracle's map), and the encodings RFC 9496
appendix A.3 says must be rejected (non-canonical field elements, negative s, non-squares, negative xy, y = 0).

Expected values come from oracle.cbind.msm_many on the job off = arange(n + 1), pidx = arange(n) -- the independent C restatement -- computed
once per process and shared; nothing here calls the code under test."""
import functools
import hashlib

import numpy as np

from oracle import cbind as C
from tests.scalar_edge_cases import HOT_W, L, VALUES, random_256
from tests.test_host_field import BAD_ENCODINGS, GENERATOR_MULTIPLES

BASEPOINT = bytes.fromhex(GENERATOR_MULTIPLES[1])
IDENTITY = bytes(32)
EDGES = [0, 1, L - 1, L, L + 1, 2**255, 2**256 - 1]
WINDOW_WIDTHS = (4, HOT_W)


def window_scalars():
    """for w in WINDOW_WIDTHS and v in (0, 1, 2^(w-1) - 1, 2^(w-1), 2^w - 1): v in every w-bit window of a 256-bit scalar (the top window cut at bit 256)"""
    out = []
    for w in WINDOW_WIDTHS:
        for v in (0, 1, (1 << (w - 1)) - 1, 1 << (w - 1), (1 << w) - 1):
            out.append(sum(v << (w * k) for k in range((256 + w - 1) // w)) & (2**256 - 1))
    return out


def scalar_values(n_random=120):
    seen, out = set(), []
    for v in VALUES + EDGES + window_scalars() + random_256(8, n_random):
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def rows(values, width=32) -> np.ndarray:
    """integers -> uint8 [n][width], little endian"""
    return np.frombuffer(b"".join(int(v).to_bytes(width, "little") for v in values), np.uint8).reshape(-1, width).copy()


def enc_rows(encodings) -> np.ndarray:
    return np.frombuffer(b"".join(encodings), np.uint8).reshape(-1, 32).copy()


BASEPOINT_ROW = enc_rows([BASEPOINT])


@functools.lru_cache(maxsize=None)
def hashed_points(n=5):
    C.build()
    return tuple(C.from_uniform_bytes(hashlib.sha512(b"point_mul_cases %d" % i).digest()) for i in range(n))


def valid_points():
    return [BASEPOINT, IDENTITY] + list(hashed_points())


def invalid_points():
    return [bytes.fromhex(h) for h in BAD_ENCODINGS]


@functools.lru_cache(maxsize=None)
def pair_operands():
    """(scalars [n][32], points [n][32], valid [n]): every scalar on a valid point (the points taken in turn), every point -- the invalid
    encodings too -- under the edge scalars, the invalid ones placed BETWEEN valid neighbours"""
    sc, pt = [], []
    good, bad = valid_points(), invalid_points()
    for i, v in enumerate(scalar_values()):
        sc.append(v)
        pt.append(good[i % len(good)])
    for j, p in enumerate(good):
        for v in EDGES + window_scalars():
            sc.append(v)
            pt.append(p)
    for j, p in enumerate(bad):                                # valid | invalid | valid: the neighbours' outputs must not change
        for k, v in enumerate((EDGES[j % len(EDGES)], 2**256 - 1 - j)):
            sc += [v, v, v]
            pt += [good[(j + k) % len(good)], p, good[(j + k + 2) % len(good)]]
    bad_set = set(bad)
    valid = np.array([p not in bad_set for p in pt])
    return rows(sc), enc_rows(pt), valid


@functools.lru_cache(maxsize=None)
def pair_expected():
    """(out [n][32], status [n]) of pair_operands() from the oracle"""
    s, p, _ = pair_operands()
    C.build()
    n = len(s)
    return C.msm_many(np.arange(n + 1, dtype=np.uint32), s, np.arange(n, dtype=np.uint32), p, 1)


@functools.lru_cache(maxsize=None)
def base_operands():
    return rows(scalar_values())


@functools.lru_cache(maxsize=None)
def base_expected():
    """[n][32]: base_operands()[i] * B from the oracle"""
    s = base_operands()
    C.build()
    n = len(s)
    out, st = C.msm_many(np.arange(n + 1, dtype=np.uint32), s, np.zeros(n, np.uint32), enc_rows([BASEPOINT]), 1)
    assert not st.any()
    return out


def tiled(a: np.ndarray, n: int) -> np.ndarray:
    """the first n rows of `a` repeated as often as needed"""
    reps = (n + len(a) - 1) // len(a)
    return np.ascontiguousarray(np.concatenate([a] * reps)[:n])
