"""(helper module of tests/test_host_msm_optional_many.py and tests/test_gpu_msm_optional_many.py)
Jobs for zkp_msm_optional_many / zkp_multiscalar_optional_batch -- many variable-time multiscalar sums with long segments -- and their expected bytes.

Points, scalars and the oracle are those of tests/msm_segments_cases.py: the 64-row catalogue, rows of a job's own ((1000 + j) B), the encodings that
do not decode, every fifth scalar a 256-bit edge value.  Segment lengths are given in terms of S, the segment length above which the call runs the
bucket method (zkp_msm_optional_many_min_segment(), read from the library by the caller and never written here).

Expected bytes and status come from oracle.cbind.msm_many (variable time) on the job itself, computed once per job.  Nothing here calls the code
under test."""
import re

import numpy as np

from tests import msm_segments_cases as MC
from tests import point_mul_cases as PC
from tests import scalar_edge_cases as SE

L = MC.L
VARTIME = 0
N_CAT = MC.N_CATALOGUE
N_OWN = 448                                    # rows of its own a job adds to the catalogue: 512 points in all


def single_lengths(S):
    """both sides of the term-path rule and of the window widths 7 | 10 (4,096 terms) and 10 | 11 (8,192)"""
    return [1, S, S + 1, 4095, 4096, 8191, 8192]


def ragged_lengths(S):
    return [0, 1, S, S + 1, 0, 300, 511, 512, 513, 1024, 1025, 4096, 5000, 0, 8199, 2]


def points512():
    """the catalogue plus N_OWN rows used by nobody else: [512][32], all valid, no two equal"""
    return np.concatenate([MC.catalogue(), MC.extra_rows(N_OWN)])


def job(lens, seed=1, points=None):
    """(off, scalars, pidx, points): segment i has lens[i] terms on points drawn from all rows of `points` (default: points512())"""
    points = points512() if points is None else points
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    t = int(off[-1])
    pidx = np.random.default_rng(seed).integers(0, len(points), size=t).astype(np.uint32)
    return off, MC.scalars(t, seed), pidx, points


def shuffled(lens, seed):
    """the lengths in a seeded order (that the classes interleave in it is the caller's assertion)"""
    order = np.random.default_rng(seed).permutation(len(lens))
    return [lens[i] for i in order]


def own_points(off, sc, pidx, points):
    return MC.own_points(off, sc, pidx, points)


def expected(name, off, sc, pidx, points):
    return MC.expected("optmany-" + name, off, sc, pidx, points, VARTIME)


def with_invalid(S, seed=5):
    """(off, scalars, pidx, points, flagged): segments of several classes and three short ones, with encodings that do not decode
      * at the first term of a long segment, at the last term of another, in the middle of the longest segment of its run,
      * ONE bad row referenced from two segments of different classes,
      * one bad row in a short segment (the term-path route)."""
    lens = [2 * S + 9, 3, 600, 2 * S + 1, S, 1300, 0, 700, 40, 3 * S]
    off, sc, pidx, pts = job(lens, seed)
    bad = MC.invalid_rows()
    points = np.concatenate([pts, bad[:5]])
    b = [len(pts) + j for j in range(5)]
    pidx = pidx.copy()
    pidx[int(off[0])] = b[0]                                # first term of segment 0
    pidx[int(off[4]) - 1] = b[1]                            # last term of segment 3
    pidx[int(off[5]) + 650] = b[2]                          # the middle of the 1,300-term segment, the longest of its run
    pidx[int(off[2]) + 17] = b[3]                           # one row, two segments: the 600-term one ...
    pidx[int(off[7]) + 100] = b[3]                          # ... and the 700-term one, which the class of 1,300 holds
    pidx[int(off[8]) + 7] = b[4]                            # the 40-term segment: the term path
    flagged = [0, 2, 3, 5, 7, 8]
    return off, sc, pidx, points, flagged, lens


def identity_cases(S):
    """(off, scalars, pidx, points, identity segments, others): all-zero scalars over S + 5 terms; s P + (l - s) P over S + 3 pairs; the scalars l, l + 1
    and 2^256 - 1 between S + 1 zero-sum pairs; the identity encoding as the only operand of S + 2 terms; and the identity among other operands"""
    pts = points512()
    ident = int(np.flatnonzero((pts == 0).all(axis=1))[0])
    s_vals = [v % L for v in SE.random_256(11, S + 3)]
    pair_sc, pair_pi = [], []
    for j, s in enumerate(s_vals):
        pair_sc += [s, L - s]
        pair_pi += [2 + j % 300, 2 + j % 300]
    edge_sc, edge_pi = [L, L + 1, 2 ** 256 - 1, 1], [0, 3, 4, 5]
    for j, s in enumerate(s_vals[:S + 1]):
        edge_sc += [s, L - s]
        edge_pi += [70 + j, 70 + j]
    id_sc = [(5 + 7 * j) if j % 3 else 2 ** 256 - 1 - j for j in range(S + 2)]
    mix_sc, mix_pi = [], []
    for j in range(S + 4):
        mix_sc.append(3 + j)
        mix_pi.append(ident if j % 2 else 0)
    segs = [([0] * (S + 5), list(range(S + 5))),
            (pair_sc, pair_pi),
            (edge_sc, edge_pi),
            (id_sc, [ident] * (S + 2)),
            (mix_sc, mix_pi)]
    off = np.concatenate([[0], np.cumsum([len(s) for s, _ in segs])]).astype(np.uint32)
    sc = PC.rows([v for s, _ in segs for v in s])
    pidx = np.array([p % len(pts) for _, pp in segs for p in pp], np.uint32)
    assert all(n > S for n in np.diff(off.astype(np.int64)))
    return off, sc, pidx, pts, [0, 1, 3], [2, 4]


def repeated_job(n_seg, seg_len, distinct, seed):
    """(off, scalars, pidx, points, which): n_seg segments of seg_len terms of which only `distinct` differ -- segment i holds the terms of segment
    which[i] = i % distinct -- so that the oracle needs `distinct` sums and not n_seg"""
    off_d, sc_d, pidx_d, pts = job([seg_len] * distinct, seed)
    which = np.arange(n_seg) % distinct
    sc = np.ascontiguousarray(sc_d.reshape(distinct, seg_len, 32)[which].reshape(-1, 32))
    pidx = np.ascontiguousarray(pidx_d.reshape(distinct, seg_len)[which].reshape(-1))
    off = (np.arange(n_seg + 1, dtype=np.uint64) * seg_len).astype(np.uint32)
    return off, sc, pidx, pts, which, (off_d, sc_d, pidx_d)


RUN_NOTE = re.compile(r"k_pip_prepare_csr<(\d+)>@K=(\d+),n=(\d+),at=(\d+)$")


def runs_of(names):
    """[(c, K, n, at)] of the runs zkp_ctx_last_kernels(ZKP_K_DECODE) names, in run order"""
    runs = []
    for nm in names:
        m = RUN_NOTE.match(nm)
        if m:
            runs.append(tuple(int(g) for g in m.groups()))
    return sorted(runs, key=lambda r: r[3])


def check_plan(runs, lens, S):
    """what the notes of a host-pointer call must say about its plan: every segment longer than S is a member of exactly one run, in falling length over
    the run order; the run's n is its longest member; NO MEMBER IS PADDED BY A FACTOR OF TWO OR MORE.  Returns the member lengths per run"""
    long_lens = sorted((n for n in lens if n > S), reverse=True)
    assert sum(r[1] for r in runs) == len(long_lens), (runs, long_lens)
    members, at = [], 0
    for c, K, n, pos in runs:
        assert pos == at, runs
        m = long_lens[at:at + K]
        assert m[0] == n and all(2 * x > n for x in m), (n, m)
        members.append(m)
        at += K
    return members
