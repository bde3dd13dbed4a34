"""(helper module of tests/test_host_msm_segments.py and tests/test_gpu_msm_segments.py)
Operands of the multiscalar sums with long segments (zkp_msm_segments, zkp_multiscalar_sum_batch) and their expected bytes.

Points: a catalogue of 64 rows -- the valid points of tests/point_sum_cases.py (B, the identity, hashed points, small multiples, negatives), then
j B for as many j as it takes, from the oracle -- and the encodings tests/point_mul_cases.py lists as invalid.  Scalars: the 256-bit edge values of
tests/scalar_edge_cases.py (0, 1, l - 1, l, l + 1, 2^256 - 1, window patterns ...) between seeded random 256-bit values.  A job is (off, scalars,
pidx, points) in CSR form; segment lengths are given in units of the fold's group size G, which the caller reads from the library.

Expected bytes and status come from oracle.cbind.msm_many on the job itself, an independent CPU restatement (8,300 terms take 0.08 s in variable
and 0.3 s in constant time), computed once per job.  Nothing here calls the code under test."""
import functools

import numpy as np

from oracle import cbind as C
from tests import point_mul_cases as PC
from tests import point_sum_cases as SC
from tests import scalar_edge_cases as SE

L = SE.L
N_CATALOGUE = 64


@functools.lru_cache(maxsize=None)
def catalogue():
    """points [64][32], every row valid and no two rows equal"""
    C.build()
    rows = list(dict.fromkeys(SC.valid_points()))
    k = N_CATALOGUE - len(rows)
    mult, st = C.msm_many(np.arange(k + 1, dtype=np.uint32), PC.rows(range(7, 7 + k)), np.zeros(k, np.uint32), PC.BASEPOINT_ROW, 0)
    assert not st.any()
    pts = np.concatenate([PC.enc_rows(rows), mult])
    assert len(pts) == N_CATALOGUE and len({bytes(r) for r in pts}) == N_CATALOGUE
    return pts


def invalid_rows():
    return PC.enc_rows(SC.invalid_points())


def scalars(t, seed):
    """[t][32]: random 256-bit values, every fifth row an edge value of the catalogue (taken in turn from a seeded start)"""
    vals = SE.random_256(seed, t)
    edges = SE.VALUES + PC.EDGES
    for j in range(0, t, 5):
        vals[j] = edges[(seed + j // 5) % len(edges)]
    return PC.rows(vals) if t else np.zeros((0, 32), np.uint8)


def job(lens, seed=1):
    """(off, scalars, pidx, points) over the catalogue: segment i has lens[i] terms"""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    t = int(off[-1])
    pidx = np.random.default_rng(seed).integers(0, N_CATALOGUE, size=t).astype(np.uint32)
    return off, scalars(t, seed), pidx, catalogue()


def own_points(off, sc, pidx, points):
    """the same job with one row per term (what pidx = None means): (off, scalars, rows [T][32])"""
    return off, sc, np.ascontiguousarray(points[pidx])


def single_lengths(G):
    return [1, G - 1, G, G + 1, 2 * G, 2 * G + 1, G * G // 2, G * G // 2 + 1, G * G, G * G + 1]


def ragged_lengths(G):
    """801 terms at G = 32: empty segments first, in the middle and last, runs that end inside a group, runs that cross two or more groups"""
    return [0, 1, G - 1, 0, G, G + 1, 1, 3 * G + 5, 0, 2, 600, 0]


def four_level_lengths(G):
    return [G ** 3 // 4 + 5, 1, 0, 2]


def with_invalid(G, seed=3):
    """(off, scalars, pidx, points, flagged segments): the ragged job plus a segment of 3 G + 7 terms, with invalid encodings at the first and at the
    last position of a group, inside the segment that spans three or more groups, and ONE invalid row referenced from two segments"""
    lens = ragged_lengths(G) + [3 * G + 7, 4, 0, 9]
    off, sc, pidx, pts = job(lens, seed)
    bad = invalid_rows()
    points = np.concatenate([pts, bad])
    b0, b1, b2, b3 = (N_CATALOGUE + j for j in range(4))
    seg_of = lambda t: int(np.searchsorted(off, t, side="right")) - 1
    long_seg = len(ragged_lengths(G))                                  # the 3 G + 7 segment
    first_of_group = (int(off[long_seg]) // G + 1) * G                 # inside the long segment
    last_of_group = first_of_group + 2 * G - 1
    assert off[long_seg] < first_of_group and last_of_group < off[long_seg + 1]
    pidx = pidx.copy()
    pidx[first_of_group] = b0
    pidx[last_of_group] = b1
    t600 = int(off[10]) + 2 * G + 3                                    # inside the 600-term segment, in the middle of a group
    pidx[t600] = b2
    shared = [int(off[4]) + 1, int(off[long_seg + 1]) + 2]             # one invalid row, two segments (the G-term one and the 4-term one)
    for t in shared:
        pidx[t] = b3
    flagged = sorted({seg_of(t) for t in [first_of_group, last_of_group, t600] + shared})
    assert len(flagged) == 4
    return off, sc, pidx, points, flagged


def special_cases(G):
    """(off, scalars, pidx, points, identity segments): an all-zero-scalar segment, s P + (l - s) P over G + 3 pairs, the scalars l, l + 1 and 2^256 - 1,
    and the identity encoding as an operand"""
    pts = catalogue()
    ident = int(np.flatnonzero((pts == 0).all(axis=1))[0])
    s_vals = SE.random_256(11, G + 3)
    pair_sc, pair_pi = [], []
    for j, s in enumerate(s_vals):
        s %= L
        pair_sc += [s, L - s]
        pair_pi += [2 + j % 5, 2 + j % 5]
    segs = [([0] * (G + 1), list(range(G + 1))),                                       # zero scalars: the identity
            (pair_sc, pair_pi),                                                         # s P + (l - s) P: the identity
            ([L, L + 1, 2 ** 256 - 1, 1], [0, 3, 4, 5]),
            ([5, 2 ** 256 - 1, L - 1], [ident, ident, ident]),                          # the identity as an operand, alone: the identity
            ([7, 9, L + 1], [ident, 0, ident])]
    off = np.concatenate([[0], np.cumsum([len(s) for s, _ in segs])]).astype(np.uint32)
    sc = PC.rows([v for s, _ in segs for v in s])
    pidx = np.array([p % N_CATALOGUE for _, pp in segs for p in pp], np.uint32)
    return off, sc, pidx, pts, [0, 1, 3]


_memo = {}


def expected(name, off, sc, pidx, points, flags):
    """the oracle's (out, status) for a job, computed once per (name, flags); pidx = None is the arange job"""
    key = (name, flags)
    if key not in _memo:
        C.build()
        pi = np.arange(int(off[-1]), dtype=np.uint32) if pidx is None else pidx
        out, st = C.msm_many(off, sc, pi, np.ascontiguousarray(points), flags)
        out.setflags(write=False)
        st.setflags(write=False)
        _memo[key] = (out, st)
    return _memo[key]
