"""(helper module of tests/test_host_scan.py and tests/test_gpu_scan.py)
Jobs for the segmented prefix sums and products of scalars and the running sums of points (zkp_sc_scan, zkp_scan_points and the toolbox calls
behind scalar_cumsum / scalar_cumprod / scalar_powers / point_cumsum) and their expected values.

Scalars: a job is (op, off, a, aidx) with a as a list of Python integers below 2^256 (any 32 bytes are an operand); expected rows are Python
integers mod l.  Points: a job is (off, pidx, neg) over a CATALOGUE of points with known logarithms, m B for small m, the identity, -B and one
encoding that does not decode; the expected row of a prefix is (the signed sum of its logarithms) B from the existing host basepoint_mul, one
multiplication per distinct prefix value, and status 1 with a zero row where the prefix holds the invalid encoding.  Nothing in this module calls
the code under test.  Lengths are given in units of the scan's group size G, which the caller reads from zkp_sc_scan_group() /
zkp_scan_points_group(); the host tests use the same lengths."""
import functools

import numpy as np

from tests.scalar_edge_cases import L, VALUES, random_256
from tests.scalar_reduce_cases import ints, offsets, rows  # noqa: F401  (re-exported)

SUM, PRODUCT = 0, 1
OPS = (SUM, PRODUCT)
MODES = (False, True)                        # exclusive?
EDGES = list(dict.fromkeys([0, 1, L - 1, L, L + 1, 2 ** 252, 2 ** 256 - 1] + VALUES))


# ---- the shapes both scans are tested on ---------------------------------------------------------------------------------------------------------
def single_lengths(G):
    return [1, 2, G - 1, G, G + 1, 2 * G, 2 * G + 1]


def shapes(G):
    """name -> segment lengths; a unit is G consecutive terms, the first begins at term 0"""
    rng = np.random.default_rng(G)
    return {
        "three_whole_units": [G - 3, 3 * G + 10, 4],            # units 1, 2 and 3 are one run each: they pass their carry on
        "boundary_at_edge": [G, G + 5],
        "boundary_before_edge": [G - 1, G + 5],
        "boundary_after_edge": [G + 1, G + 5],
        "ones_across_edge": [G - 4] + [1] * 8 + [G],
        "empties": [0, 0, 5, 0, G, 0, 0, 0, 7, G + 1, 0, 0],
        "ragged": [int(v) for v in rng.integers(0, 2 * G // 3, size=14)] + [2 * G + 1, 0, 3],
        "one_unit_ragged": [0, 3, 0, G // 2, 1, 1, G // 4, 0],  # everything inside unit 0: no carry anywhere
        "segments_that_are_whole_units": [G, G, 0, G, 5],       # several units, every segment begins at a unit edge: no carry anywhere
    }


def multi_unit(lens, G):
    """does a segment of the job cross a unit edge (so that a carry is needed)?"""
    off = offsets(lens)
    return any(int(off[i + 1]) > int(off[i]) and int(off[i]) // G != (int(off[i + 1]) - 1) // G for i in range(len(lens)))


def launch_edges(launches_fn, limit=1 << 22):
    """[(launch count, smallest T with it)] for every launch count a T <= limit has, by bisection on the library's *_launches function"""
    out = [(launches_fn(1), 1)]
    top = launches_fn(limit)
    while out[-1][0] < top:
        lo, hi = out[-1][1], limit                  # launches(lo) == out[-1][0] < launches(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if launches_fn(mid) > out[-1][0]:
                hi = mid
            else:
                lo = mid
        out.append((launches_fn(hi), hi))
    return out


# ---- scalars -------------------------------------------------------------------------------------------------------------------------------------
def sc_expected(op, off, a, aidx=None, exclusive=False):
    """the integers mod l of every row"""
    out = []
    for s in range(len(off) - 1):
        acc = 1 if op == PRODUCT else 0
        for t in range(int(off[s]), int(off[s + 1])):
            x = a[t if aidx is None else int(aidx[t])]
            nxt = acc * x % L if op == PRODUCT else (acc + x) % L
            out.append(acc if exclusive else nxt)
            acc = nxt
    return out


def sc_operands(op, t, seed):
    """t random 256-bit integers; factors stay non-zero so that a wrong factor shows in every later row"""
    a = random_256(seed, t)
    return [v if v % L else 3 for v in a] if op == PRODUCT else a


def sc_job(op, lens, seed=1):
    off = offsets(lens)
    return op, off, sc_operands(op, int(off[-1]), seed), None


def sc_edge_rotation(op, G, shift):
    """segments [G - 2, G + 7, 3]: the catalogue's values from term 0 on, rotated by `shift`; a zero is a legitimate factor here"""
    op, off, a, _ = sc_job(op, [G - 2, G + 7, 3], seed=50 + shift)
    for k in range(len(a)):
        if k % 3 != 2:                               # (every third operand stays random)
            a[k] = EDGES[(k + shift) % len(EDGES)]
    return op, off, a, None


def sc_zero_factor(G, p):
    """segments [G, 2 G + 3, 5] of non-zero factors, a zero (0, l or 2 l) at position p of the long one"""
    op, off, a, _ = sc_job(PRODUCT, [G, 2 * G + 3, 5], seed=70 + p)
    a[G + p] = [0, L, 2 * L][p % 3]
    return op, off, a, None


def sc_gathers(op, G):
    """index lists that repeat and skip rows: all indices one row; every other row, backwards; random rows"""
    rng = np.random.default_rng(17 + op)
    a = sc_operands(op, 11, 90)
    off = offsets([0, 1, G + 2, 3, G])
    t = int(off[-1])
    return [(op, off, a, np.full(t, 4, np.uint32)), (op, off, a, (10 - 2 * (np.arange(t) % 5)).astype(np.uint32)),
            (op, off, a, rng.integers(0, 11, size=t).astype(np.uint32))]


def with_arange(jb):
    op, off, a, aidx = jb
    return op, off, a, np.arange(int(off[-1]), dtype=np.uint32) if aidx is None else aidx


# ---- points --------------------------------------------------------------------------------------------------------------------------------------
LOGS = (1, 2, 3, 5, 8, 13, 0, -1)            # catalogue rows 0 .. 7: m B; row 6 is the identity, row 7 is -B; consecutive rows 0 .. 5 add up to the next
IDENTITY_ROW, BAD_ROW = 6, 8


def multiples(values):
    """{m: encode(m B)} from the existing host backend (toolbox.basepoint_mul with eng = None), one multiplication per distinct value"""
    from zkp_amd import toolbox as T
    vals = sorted({int(v) % L for v in values})
    enc = T.basepoint_mul(None, rows(vals)) if vals else np.zeros((0, 32), np.uint8)
    return {v: enc[i] for i, v in enumerate(vals)}


@functools.lru_cache(maxsize=None)
def catalogue():
    """points uint8 [9][32]: LOGS[i] B for the rows 0 .. 7 and, as row BAD_ROW, an encoding that does not decode"""
    from tests.point_mul_cases import invalid_points
    m = multiples(LOGS)
    pts = np.stack([m[v % L] for v in LOGS] + [np.frombuffer(invalid_points()[1], np.uint8)])
    assert not pts[IDENTITY_ROW].any()
    return np.ascontiguousarray(pts)


def pt_prefix_logs(off, pidx, neg, exclusive):
    """(signed sum of logarithms int64 [T], bad bool [T]) of every row, by cumulative sums over the whole axis less their value at the segment's start"""
    off = np.asarray(off, np.int64)
    t = int(off[-1])
    pidx = np.asarray(pidx, np.int64)
    sign = np.ones(t, np.int64) if neg is None else 1 - 2 * (np.asarray(neg) != 0).astype(np.int64)
    bad = pidx == BAD_ROW
    logs = np.where(bad, 0, np.array(LOGS + (0,), np.int64)[pidx]) * sign
    lens = np.diff(off)
    start = np.repeat(off[:-1], lens)               # the first term of each term's segment
    cs, cb = np.concatenate([[0], np.cumsum(logs)]), np.concatenate([[0], np.cumsum(bad)])
    upto = np.arange(t) + (0 if exclusive else 1)
    return cs[upto] - cs[start], (cb[upto] - cb[start]) > 0


def pt_expected(off, pidx, neg=None, exclusive=False):
    """(out uint8 [T][32], status uint8 [T])"""
    logs, bad = pt_prefix_logs(off, pidx, neg, exclusive)
    if len(logs) == 0:
        return np.zeros((0, 32), np.uint8), np.zeros(0, np.uint8)
    values, inverse = np.unique(logs, return_inverse=True)
    m = multiples(values)
    out = np.stack([m[int(v) % L] for v in values])[inverse.reshape(-1)]
    out[bad] = 0
    return np.ascontiguousarray(out), bad.astype(np.uint8)


def pt_job(lens, seed=1, bad_at=()):
    """(off, pidx, neg): random valid rows of the catalogue with mixed signs; the terms listed in bad_at reference the invalid row"""
    rng = np.random.default_rng(seed)
    off = offsets(lens)
    t = int(off[-1])
    pidx = rng.integers(0, BAD_ROW, size=t).astype(np.uint32)
    neg = (rng.integers(0, 3, size=t) == 0).astype(np.uint8)
    for p in bad_at:
        pidx[p] = BAD_ROW
    return off, pidx, neg


def pt_triples(t, lens=None):
    """(off, pidx, neg) of t terms whose prefixes take few values however long the job is: +f_i B, +f_(i+1) B, -f_(i+2) B over the Fibonacci rows of the
    catalogue, so that a prefix is 0, f_i or f_(i+2) -- and is NOT zero at two of three unit edges, where a lost carry shows"""
    k = np.arange(t)
    i = (k // 3) % 4
    pidx = (i + k % 3).astype(np.uint32)
    neg = (k % 3 == 2).astype(np.uint8)
    return offsets([t] if lens is None else lens), pidx, neg
