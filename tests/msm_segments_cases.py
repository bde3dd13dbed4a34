"""(helper module of tests/test_host_msm_segments.py and tests/test_gpu_msm_segments.py)
Operands of the multiscalar sums with long segments (zkp_msm_segments, zkp_multiscalar_sum_batch) and their expected bytes.

Points: a catalogue of 64 rows -- the valid points of tests/point_sum_cases.py (B, the identity, hashed points, small multiples, negatives), then
j B for as many j as it takes, from the oracle -- and the encodings tests/point_mul_cases.py lists as invalid.  Scalars: the 256-bit edge values of
tests/scalar_edge_cases.py (0, 1, l - 1, l, l + 1, 2^256 - 1, window patterns ...) between seeded random 256-bit values.  A job is (off, scalars,
pidx, points) in CSR form; segment lengths are given in units of the fold's group size G, which the caller reads from the library.

Those jobs give every point dozens of uses.  The jobs of the second half (own_rows_job, mixed_job, mixed_job_with_invalid, many_segments_job) add rows
(1000 + j) B of their own, used once or exactly twice, next to the catalogue, so that a call of 1,024 terms or more has terms in every class of the
classified term path: registered fixed-base points, comb tables of shared points, the smallest comb table (two uses) and single-use points.

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


# ---- jobs for every class of the classified term path (1,024 terms or more): registered fixed-base points, points with a comb table (many uses, or
#      exactly two), single-use points (the ladder in variable time; a comb table of their own, or the constant-time ladder, in constant time) ----------
EDGE_SCALARS = list(dict.fromkeys(SE.VALUES + PC.EDGES))
REGISTERED = tuple(range(2, 13))              # the 11 catalogue rows the tests hand to prepare_fixed_points (hashed points, small multiples, negatives)
CLASS_REGISTERED, CLASS_SHARED, CLASS_TWICE, CLASS_ONCE = 0, 1, 2, 3
CLASS_NAMES = ("registered", "shared", "twice", "once")
EXTRA_FIRST_LOG, N_EXTRA = 1000, 4096


def threshold(const):
    """the value of a size threshold of the term path, from the table tests/test_host_size_thresholds.py ties to the sources"""
    from tests import size_thresholds as S
    values = {r["value"] for r in S.ROWS if r["const"] == const}
    assert len(values) == 1, (const, values)
    return values.pop()


@functools.lru_cache(maxsize=None)
def _extra_rows():
    """[4096][32]: (1000 + j) B from the oracle, none of them a catalogue row"""
    C.build()
    logs = np.arange(EXTRA_FIRST_LOG, EXTRA_FIRST_LOG + N_EXTRA)
    pts, st = C.msm_many(np.arange(N_EXTRA + 1, dtype=np.uint32), PC.rows(logs), np.zeros(N_EXTRA, np.uint32), PC.BASEPOINT_ROW, 0)
    assert not st.any() and len({bytes(r) for r in pts} | {bytes(r) for r in catalogue()}) == N_EXTRA + N_CATALOGUE
    pts.setflags(write=False)
    return pts


def extra_rows(n):
    assert n <= N_EXTRA
    return _extra_rows()[:n].copy()


def own_rows_job(T, seed=1):
    """(off, scalars, rows [T][32], logs [T]): ONE segment of T terms with a row per term (pidx = None).  Row t is d_t B with d_0 = 0 (the identity),
    d_1 = 1 (B itself) and d_t = 1000 + t - 2 after that: valid, no two equal, every point used once.  Every fifth scalar is an edge value"""
    assert T >= 2
    rows = np.concatenate([PC.enc_rows([PC.IDENTITY, PC.BASEPOINT]), extra_rows(T - 2)])
    logs = [0, 1] + list(range(EXTRA_FIRST_LOG, EXTRA_FIRST_LOG + T - 2))
    assert len(rows) == T and len({bytes(r) for r in rows}) == T
    return np.array([0, T], np.uint32), scalars(T, seed), rows, logs


def mixed_lengths(G, total):
    """ragged_lengths(G) + [G G / 2 + 1, 0, 3, 2 G + 1], then segments of G + 1 terms (the last one cut) up to `total` terms exactly; a smaller `total`
    leaves the 1,382 terms (G = 32) of the fixed part"""
    lens = ragged_lengths(G) + [G * G // 2 + 1, 0, 3, 2 * G + 1]
    while sum(lens) < total:
        lens.append(min(G + 1, total - sum(lens)))
    return lens


def _seg_of(off, t):
    return int(np.searchsorted(off, t, side="right")) - 1


@functools.lru_cache(maxsize=None)
def _mixed(G, total, seed):
    lens = mixed_lengths(G, total)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    T = int(off[-1])
    assert T >= total and (T == total or len(lens) == len(ragged_lengths(G)) + 4)
    rng = np.random.default_rng(seed)
    cat = catalogue()
    # classes in turn, so that every segment border falls between two classes ...
    cls = (np.arange(T) % 4).astype(np.int64)
    # ... but for two segments that cancel to the identity: the 2-term one on a single-use point (two rows of the same bytes, each used once), the
    # 3-term one on a shared point
    seg_once, seg_shared = 9, len(ragged_lengths(G)) + 2
    assert lens[seg_once] == 2 and lens[seg_shared] == 3
    t_once, t_shared = int(off[seg_once]), int(off[seg_shared])
    cls[t_once:t_once + 2] = CLASS_ONCE
    cls[t_shared:t_shared + 3] = CLASS_SHARED
    twice = np.flatnonzero(cls == CLASS_TWICE)
    if len(twice) % 2:                                               # (a point used twice needs two terms)
        cls[twice[-1]] = CLASS_SHARED
        twice = twice[:-1]
    once = np.flatnonzero(cls == CLASS_ONCE)
    n_pairs, n_once = len(twice) // 2, len(once)
    S = n_pairs + n_once
    points = np.concatenate([cat, extra_rows(S)])
    shared = np.array([p for p in range(N_CATALOGUE) if p not in REGISTERED], np.uint32)
    pidx = np.zeros(T, np.uint32)
    reg_terms, shared_terms = np.flatnonzero(cls == CLASS_REGISTERED), np.flatnonzero(cls == CLASS_SHARED)
    pidx[reg_terms] = np.array(REGISTERED, np.uint32)[rng.permutation(len(reg_terms)) % len(REGISTERED)]
    pidx[shared_terms] = shared[rng.permutation(len(shared_terms)) % len(shared)]                       # (every shared row the same number of uses, +- 1)
    pidx[rng.permutation(twice)] = N_CATALOGUE + np.repeat(np.arange(n_pairs, dtype=np.uint32), 2)      # the two uses of a point lie anywhere in the job
    pidx[once] = N_CATALOGUE + n_pairs + np.arange(n_once, dtype=np.uint32)
    vals = SE.random_256(seed, T)
    fixed = set()                                                    # terms whose scalar or row has a role of its own
    # s P + (l - s) P on two single-use rows of the same bytes; s1 P + s2 P + (l - s1 - s2) P on one shared point
    s = vals[t_once] % L
    vals[t_once], vals[t_once + 1] = s, L - s
    points[pidx[t_once + 1]] = points[pidx[t_once]]
    s1, s2 = vals[t_shared] % L, vals[t_shared + 1] % L
    vals[t_shared:t_shared + 3] = [s1, s2, (2 * L - s1 - s2) % L]
    pidx[t_shared:t_shared + 3] = shared[5]
    fixed |= {t_once, t_once + 1, t_shared, t_shared + 1, t_shared + 2}
    # one single-use row carries the bytes of a point the test registers: k_hot_match compares bytes, so this term takes the fixed-base walk
    t_hot = int(once[len(once) // 2])
    assert t_hot not in fixed
    points[pidx[t_hot]] = cat[REGISTERED[0]]
    # every edge scalar in every class: on every second free term of the class
    for c in range(4):
        slots = [int(t) for t in np.flatnonzero(cls == c) if t not in fixed][0::2]
        assert len(slots) >= len(EDGE_SCALARS), "class %s has %d slots for %d edge scalars: raise the job's size" % (CLASS_NAMES[c], len(slots), len(EDGE_SCALARS))
        for j, t in enumerate(slots):
            vals[t] = EDGE_SCALARS[j % len(EDGE_SCALARS)]
    sc = PC.rows(vals)
    # what the job holds, checked on the arrays themselves
    uses = np.bincount(pidx, minlength=len(points))
    assert len(points) == N_CATALOGUE + S and (uses[N_CATALOGUE:N_CATALOGUE + n_pairs] == 2).all() and (uses[N_CATALOGUE + n_pairs:] == 1).all()
    assert (uses[list(REGISTERED)] >= 10).all() and (uses[shared] >= 5).all()
    for c in range(4):
        have = {vals[t] for t in np.flatnonzero(cls == c)}
        assert set(EDGE_SCALARS) <= have, CLASS_NAMES[c]
    assert set(cls[pidx < N_CATALOGUE]) == {CLASS_REGISTERED, CLASS_SHARED} and all(
        (pidx[t] in REGISTERED) == (cls[t] == CLASS_REGISTERED) for t in np.flatnonzero(pidx < N_CATALOGUE))
    empty = np.flatnonzero(np.diff(off.astype(np.int64)) == 0).tolist()
    assert empty[0] == 0 and len(empty) == 5 and lens[-1] > 0        # empty segments first and between others; the last segment ends at the last term
    info = dict(cls=cls, registered=REGISTERED, n_pairs=n_pairs, n_once=n_once, t_hot=t_hot, identity=sorted(empty + [seg_once, seg_shared]),
                counts={CLASS_NAMES[c]: int((cls == c).sum()) for c in range(4)})
    for a in (off, sc, pidx, points, cls):
        a.setflags(write=False)
    return off, sc, pidx, points, info


def mixed_job(G, total, seed=21):
    """(off, scalars, pidx, points [64 + S][32], info): at least `total` terms over the catalogue and S rows of their own, the terms taking four
    classes in turn: a) one of the 11 catalogue rows REGISTERED, b) one of the other 53 (dozens of uses each), c) a row used exactly twice in the whole
    job, d) a row used exactly once.  Every edge scalar (tests/scalar_edge_cases.py, tests/point_mul_cases.py) occurs in every class; one single-use
    row holds the bytes of a registered point; two segments cancel to the identity.  info: cls [T] (the class of every term), registered, n_pairs,
    n_once, t_hot (the term on the row with registered bytes), identity (the segments whose sum is the identity: empty or cancelling), counts"""
    return _mixed(G, total, seed)


def mixed_job_with_invalid(G, total, seed=21):
    """(off, scalars, pidx, points, flagged segments, info): mixed_job with an encoding that does not decode in each of the classes b, c and d -- b: a
    new row that six shared terms of two segments use (three each); c: the row of a point used twice; d: the row of a point used once.  Every one of
    these terms has valid terms on both sides in its segment"""
    off, sc, pidx, points, info = _mixed(G, total, seed)
    cls = info["cls"]
    bad = invalid_rows()
    points, pidx = np.concatenate([points, bad[:1]]), pidx.copy()
    b_row = len(points) - 1
    inner = lambda t: off[_seg_of(off, t)] < t < off[_seg_of(off, t) + 1] - 1          # not the first and not the last term of its segment
    free = lambda t: inner(t) and t != info["t_hot"] and _seg_of(off, t) not in info["identity"]
    seg_a, seg_b = 7, 10                                             # the 3 G + 5 segment and the 600-term one
    b_terms = [[int(t) for t in np.flatnonzero(cls == CLASS_SHARED) if off[s] < t < off[s + 1] - 1][1:4] for s in (seg_a, seg_b)]
    assert all(len(x) == 3 for x in b_terms)
    for t in b_terms[0] + b_terms[1]:
        pidx[t] = b_row
    big = len(ragged_lengths(G))                                     # the G G / 2 + 1 segment: the twice-used point has a use in it
    c_pt = next(int(pidx[t]) for t in np.flatnonzero(cls == CLASS_TWICE) if _seg_of(off, t) == big and all(
        free(int(u)) and _seg_of(off, int(u)) not in (seg_a, seg_b) for u in np.flatnonzero(pidx == pidx[t])))
    c_terms = [int(u) for u in np.flatnonzero(pidx == c_pt)]
    points[c_pt] = bad[1]
    d_term = next(int(t) for t in np.flatnonzero(cls == CLASS_ONCE) if _seg_of(off, t) == 5 and free(int(t)))       # the G + 1 segment
    points[pidx[d_term]] = bad[2]
    flagged = sorted({_seg_of(off, t) for t in b_terms[0] + b_terms[1] + c_terms + [d_term]})
    assert len(c_terms) == 2 and 4 <= len(flagged) <= 5 and not set(flagged) & set(info["identity"])
    bad_points = {b_row, c_pt, int(pidx[d_term])}
    for t in b_terms[0] + b_terms[1] + c_terms + [d_term]:           # set between valid neighbours
        assert int(pidx[t - 1]) not in bad_points and int(pidx[t + 1]) not in bad_points
    pidx.setflags(write=False)
    points.setflags(write=False)
    return off, sc, pidx, points, flagged, info


def many_segments_job(n_msm, seed=31):
    """(off, scalars, pidx, points): n_msm segments of 1, 2, 3, 0, 1, ... terms; three of every four terms lie on the 64 catalogue rows, every fourth
    on a row of its own"""
    lens = np.resize(np.array([1, 2, 3, 0]), n_msm)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    T = int(off[-1])
    pidx = np.random.default_rng(seed).integers(0, N_CATALOGUE, size=T).astype(np.uint32)
    own = np.arange(3, T, 4)
    pidx[own] = N_CATALOGUE + np.arange(len(own), dtype=np.uint32)
    return off, scalars(T, seed), pidx, np.concatenate([catalogue(), extra_rows(len(own))])


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
