"""(helper module of tests/test_host_point_sum.py and tests/test_gpu_point_sum.py)
Operands of the batched point sums (zkp_add_points, zkp_sum_points) and their expected encodings from the oracle.

Points come from tests/point_mul_cases.py: the basepoint, the identity, hashed points, RFC 9496's multiples of the generator and the encodings that
must be rejected.  Pairs: every valid point with every other, plus (P, P), (P, -P), (P, 0), (0, P), (0, 0) and (bad, P), (P, bad), (bad, bad), with
the pairs that hold an invalid encoding rotated to the front and set BETWEEN valid ones, so that the smallest sizes hold them and neighbours show
any damage.  Expected pair values come from oracle.model's big integers (ristretto_encode(pt_add(a, +-b))).

Segments reference a small CATALOGUE through pidx, so the expected bytes of a sum of any length are one small oracle.cbind.msm_many over the
catalogue with each point's net signed multiplicity mod l as its scalar.  Nothing here calls the code under test."""
import functools

import numpy as np

from oracle import cbind as C
from oracle import model as M
from tests import point_mul_cases as PC
from tests.scalar_edge_cases import L
from tests.test_host_field import GENERATOR_MULTIPLES

ADD, SUB = 0, 1


def negated(enc: bytes) -> bytes:
    return M.ristretto_encode(M.pt_neg(M.ristretto_decode(enc)))


@functools.lru_cache(maxsize=None)
def valid_points():
    """B, the identity, hashed points, 2B .. 5B, and the negatives of two of them"""
    base = PC.valid_points() + [bytes.fromhex(h) for h in GENERATOR_MULTIPLES[2:6]]
    return tuple(base + [negated(base[0]), negated(base[3])])


def invalid_points():
    return PC.invalid_points()


@functools.lru_cache(maxsize=None)
def pair_operands():
    """(a [n][32], b [n][32], valid [n])"""
    good, bad = list(valid_points()), invalid_points()
    zero = PC.IDENTITY
    plain = [(p, q) for p in good for q in good]                       # includes (P, P), (P, -P), (P, 0), (0, P), (0, 0)
    for p in good[:4]:
        plain += [(p, p), (p, negated(p)), (p, zero), (zero, p), (zero, zero)]
    front = []
    for j, x in enumerate(bad):                                        # invalid | valid | invalid | valid ...
        p = good[j % len(good)]
        front += [(x, p), plain[3 * j], (p, x), plain[3 * j + 1], (x, bad[(j + 1) % len(bad)]), plain[3 * j + 2]]
    pairs = front + plain
    bad_set = set(bad)
    valid = np.array([a not in bad_set and b not in bad_set for a, b in pairs])
    return PC.enc_rows([a for a, _ in pairs]), PC.enc_rows([b for _, b in pairs]), valid


@functools.lru_cache(maxsize=None)
def pair_expected(op):
    """(out [n][32], status [n]) of pair_operands() under op, from the big-integer model; each distinct pair is computed once"""
    a, b, _ = pair_operands()
    memo, out, st = {}, [], []
    for ra, rb in zip(a, b):
        key = (bytes(ra), bytes(rb))
        if key not in memo:
            p, q = M.ristretto_decode(key[0]), M.ristretto_decode(key[1])
            memo[key] = None if p is None or q is None else M.ristretto_encode(M.pt_add(p, M.pt_neg(q) if op == SUB else q))
        out.append(memo[key] or bytes(32))
        st.append(memo[key] is None)
    return PC.enc_rows(out), np.array(st, np.uint8)


@functools.lru_cache(maxsize=None)
def catalogue():
    """(points [k][32], index of the one invalid row): the valid points, one invalid encoding in the middle"""
    good = list(valid_points())
    rows = good[:6] + [invalid_points()[1]] + good[6:]
    return PC.enc_rows(rows), 6


def segments_expected(off, pidx, neg, points):
    """(out [n_sums][32], status [n_sums]) of the sums of points[pidx[t]] with signs neg[t] from the oracle's msm_many: per sum one term for every
    point it references, whose scalar is the point's net signed multiplicity mod l.  points is a catalogue: the cost does not depend on the
    lengths of the sums."""
    C.build()
    off = np.asarray(off, np.int64)
    n_sums, k = len(off) - 1, len(points)
    seg = np.repeat(np.arange(n_sums), np.diff(off))
    sign = np.ones(len(seg), np.int64) if neg is None else 1 - 2 * (np.asarray(neg) != 0).astype(np.int64)
    net = np.zeros((n_sums, k), np.int64)
    used = np.zeros((n_sums, k), bool)
    np.add.at(net, (seg, np.asarray(pidx, np.int64)), sign)
    used[seg, np.asarray(pidx, np.int64)] = True
    s_idx, p_idx = np.nonzero(used)                                    # (row-major: sorted by sum)
    o = np.concatenate([[0], np.cumsum(used.sum(axis=1))]).astype(np.uint32)
    sc = PC.rows([int(v) % L for v in net[s_idx, p_idx]]) if len(s_idx) else np.zeros((0, 32), np.uint8)
    return C.msm_many(o, sc, p_idx.astype(np.uint32), np.ascontiguousarray(points), 0)


def as_msm_job(off, pidx, neg):
    """the unit-scalar job callers built before: scalars 1 / l - 1 per term"""
    one, minus = PC.rows([1])[0], PC.rows([L - 1])[0]
    t = int(off[-1])
    sc = np.tile(one, (t, 1))
    if neg is not None:
        sc[np.asarray(neg) != 0] = minus
    return np.ascontiguousarray(sc)


def ragged_job(c, seed=9, cycles=5):
    """(off, pidx, neg): lengths cycle through 0, 1, 2, c - 1, c, c + 1, 2c, 2c + 1; empty segments first, last and doubled; one segment in the
    middle of a group references the invalid row of the catalogue; signs are mixed"""
    rng = np.random.default_rng(seed)
    pts, bad = catalogue()
    lens = [0, 0] + [v for _ in range(cycles) for v in (0, 1, 2, c - 1, c, c + 1, 2 * c, 2 * c + 1)] + [3, 0, 0, 5, 0]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    t = int(off[-1])
    pidx = rng.integers(0, len(pts) - 1, size=t)
    pidx[pidx >= bad] += 1                                             # valid rows only ...
    flagged = [i for i, v in enumerate(lens) if v == 2 and 0 < off[i] % c < c - 2][-1]
    pidx[int(off[flagged]) + 1] = bad                                  # ... but for one term of one short segment inside a group
    neg = (rng.integers(0, 3, size=t) == 0).astype(np.uint8)
    return off, pidx.astype(np.uint32), neg, flagged


def single_segment(t, seed=1):
    """(off, pidx, neg) of one sum of t terms over the valid rows of the catalogue, signs mixed"""
    rng = np.random.default_rng(seed + t)
    pts, bad = catalogue()
    pidx = rng.integers(0, len(pts) - 1, size=t)
    pidx[pidx >= bad] += 1
    neg = (rng.integers(0, 4, size=t) == 0).astype(np.uint8)
    return np.array([0, t], np.uint32), pidx.astype(np.uint32), neg


def plan_levels(t, c):
    """the number of fold levels a sum job of t terms runs: n -> 2 ceil(n / c) while n > c, plus the level that finishes"""
    levels = 1
    while t > c:
        t = 2 * ((t + c - 1) // c)
        levels += 1
    return levels
