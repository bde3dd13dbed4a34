"""(helper module of tests/test_host_msm_optional_many_edges.py and tests/test_gpu_msm_optional_many_edges.py)
Jobs for zkp_msm_optional_many / _dev whose scalars are CHOSEN: bucket sizes at every step of the part count, several huge buckets in one block of the
merge, the digit-edge catalogue in slots of a K-wide run, K on both sides of the merge rule with skewed members, and the _dev form's chunking.

The jobs of tests/msm_optional_many_cases.py (OC) draw their scalars from MC.scalars: random values spread evenly over the buckets, so a bucket of a
K-wide run has one part and the merge never loops.  Here a scalar d < 2^(c-1) has the single signed digit d in window 0 (SE.pip_digits), and l - d
folds to the same bucket with the other sign: `count` copies make a bucket of exactly `count` entries.

  A  catalogue_job(c)     six segments of one class, the digit-edge values of SE.CATALOGUE for recoder pip{c} at the slots where a lane's neighbour is
                          another 256-lane block (255 | 256), the segment's first slot, and the last real slot in front of the padding
  B  ladder_job(c)        buckets of L, L + 1, 2 L, 2 L + 1, L^2 + 1, 17^2, 17^2 + 1, (4 L)^2, (4 L)^2 + 1, 128 * 4 L and 128 * 4 L + 1 entries (as many as a
                          segment of width c holds), next to a random member and a padded one
  C1 twin_huge_job()      every scalar of a segment 2^10 at c = 11: two buckets of more than kMergeSeqParts parts in ONE block of k_pip_bucket_merge
  C2 threshold_job(c, K)  K equal segments, K * W1 * B1 on either side of MERGE_LANE_MIN_BUCKETS, skewed members first, in the middle and last
  D  dev_chunk_job, dev_long_member_job, dev_term_path_job: the _dev promises of include/zkp_mi355x.h (14)

S (zkp_msm_optional_many_min_segment()) is read from the library by the caller.  The part length L, kMergeSeqParts and MERGE_LANE_MIN_BUCKETS are read
from the sources; part_len() below restates the device function of the same name.  Expected bytes and status come from OC.expected (the C oracle's
msm_many on the job itself); repeated segments go through OC.repeated_job so that the oracle sums the distinct ones only.  Nothing here calls the
code under test."""
import functools
import itertools
import math
import os
import re

import numpy as np

from tests import msm_optional_many_cases as OC
from tests import msm_segments_cases as MC
from tests import point_mul_cases as PC
from tests import scalar_edge_cases as SE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_ORDER = OC.L
WIDTHS = (7, 10, 11)
LONGEST = {7: 300, 10: 4096, 11: 8192}                    # catalogue_job: the smallest run length of widths 10 and 11, and 300 terms at c = 7


@functools.lru_cache(maxsize=None)
def _kernels():
    return open(os.path.join(ROOT, "zkp_amd", "csrc", "zkp_kernels.hip")).read()


def _source_int(pattern):
    m = re.search(pattern, _kernels())
    assert m, pattern
    return int(m.group(1))


def part_L():
    """pip_part_len(n) for n < 2^18: the least entries of a part"""
    return _source_int(r"inline uint32_t pip_part_len\(uint64_t n\) \{ return n < \(1u << 18\) \? (\d+)u :")


def merge_seq_parts():
    return _source_int(r"constexpr uint32_t kMergeSeqParts = (\d+);")


def merge_lane_min_buckets():
    return 1 << _source_int(r"constexpr size_t MERGE_LANE_MIN_BUCKETS = \(size_t\)1 << (\d+);")


def W1(c):
    """pip_cfg<C>::W1: the windows of a run of width c, the carry window included"""
    return (256 + c - 1) // c + 1


def B1(c):
    """pip_cfg<C>::B1: bucket indices 0 .. 2^(c-1) of a window"""
    return (1 << (c - 1)) + 1


def pick_c(n):
    """the window width of a run of n slots below 2^21 (pick_c of zkp_kernels.hip, restated: the tests read the width a run HAD from its note)"""
    return 7 if n < 4096 else 10 if n < 8192 else 11


def part_len(cnt):
    """part_len(cnt, L) of zkp_kernels.hip: clamp(ceil(sqrt(cnt)), L, 4 L)"""
    L = part_L()
    r = math.isqrt(cnt - 1) + 1 if cnt else 0
    return min(max(r, L), 4 * L)


def part_count(cnt):
    return -(-cnt // part_len(cnt))


def count_edges():
    """the bucket sizes at which the part count or the part length moves: L, L + 1, 2 L, 2 L + 1, L^2 + 1, (L + 1)^2, (L + 1)^2 + 1, (4 L)^2, (4 L)^2 + 1,
    kMergeSeqParts * 4 L and one more (the first bucket the whole block sums)"""
    L, big = part_L(), merge_seq_parts()
    return [L, L + 1, 2 * L, 2 * L + 1, L * L + 1, (L + 1) ** 2, (L + 1) ** 2 + 1, (4 * L) ** 2, (4 * L) ** 2 + 1, big * 4 * L, big * 4 * L + 1]


def neg(v):
    """l - v, the partner the sign fold maps onto v's digits (v <= l); -v mod l above l, where there is no such partner"""
    return L_ORDER - v if v <= L_ORDER else (L_ORDER - v) % L_ORDER


def _off(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)


def _pidx(t, seed, n_points):
    return np.random.default_rng(seed).integers(0, n_points, size=t).astype(np.uint32)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- A. the digit-edge catalogue in slots of a K-wide run --------------------------------------------------------------------------------------------
def catalogue_base(c):
    """the values of SE.CATALOGUE that name recoder pip{c} (first: they take the slots named above), then those that name no recoder (0, l +- 1,
    2^256 - 1, ...)"""
    tag = "pip%d:" % c
    own = [v for name, v in SE.CATALOGUE if tag in name]
    plain = [v for name, v in SE.CATALOGUE if ":" not in name.split("=")[0]]        # (a small construction of another recoder may share the value: "2=r4:bot_min")
    assert len(own) >= 10 and len(plain) >= 30, (len(own), len(plain))
    return list(dict.fromkeys(own + plain))


def catalogue_values(c):
    """catalogue_base(c) and l - v for each; no value twice"""
    vals = catalogue_base(c)
    return list(dict.fromkeys(vals + [neg(v) for v in vals]))


def catalogue_lens(c):
    """six segments, every one more than half the longest, one of exactly n // 2 + 1 terms (151 at c = 7: no longer than S = 192, so that member takes the
    term path of the same call and the run's shortest member is the one of 200 terms)"""
    n = LONGEST[c]
    lens = [n, n // 2 + 1, n - 1, 257, 256, 200] if c == 7 else [n, n // 2 + 1, n - 1, n // 2 + 257, 3 * n // 4, n]
    assert max(lens) == n and all(2 * x > n for x in lens) and pick_c(n) == c
    return lens


@functools.lru_cache(maxsize=None)
def catalogue_job(c):
    """(off, scalars, pidx, points, placed): MC.scalars everywhere but in the slots of `placed` = {value: [(segment, slot), ...]}.  Every segment hands out
    its slots 0, 255, 256 and its last one first, then slots spread over its whole length; value k goes to segment k % 6 and to another one"""
    lens = catalogue_lens(c)
    off, sc, pidx, pts = OC.job(lens, seed=70 + c)
    sc = sc.copy()
    vals = catalogue_values(c)
    slots = []
    for n in lens:
        special = [s for s in (0, 255, 256, n - 1) if s < n]
        special = list(dict.fromkeys(special))
        rest = [s for s in range(7, n - 1, max(1, n // 48)) if s not in special]
        slots.append(special + rest)
    placed = {v: [] for v in vals}
    for turn in range(2):
        for k, v in enumerate(vals):
            sg = k % 6 if turn == 0 else (k % 6 + 1 + (k // 6) % 5) % 6
            slot = slots[sg].pop(0)
            sc[int(off[sg]) + slot] = PC.rows([v])[0]
            placed[v].append((sg, slot))
    return _frozen(off, sc, pidx, pts) + (placed,)


# ---- B. the bucket-size ladder ----------------------------------------------------------------------------------------------------------------------
LADDER_FIRST_D = 3                                        # bucket indices 3, 4, ... in the order of count_edges(); LADDER_EMPTY_D stays empty
LADDER_EMPTY_D = 7


def ladder_counts(c):
    """[{bucket index d: entries}] per ladder segment: every count up to (L + 1)^2 + 1 in each of them; from c = 10 on (4 L)^2 in the first and (4 L)^2 + 1
    in the second; at c = 11 also kMergeSeqParts * 4 L in the first and one more in the second"""
    edges = count_edges()
    small, mid, huge = edges[:7], edges[7:9], edges[9:]
    ds = [d for d in range(LADDER_FIRST_D, LADDER_FIRST_D + len(small) + 3) if d != LADDER_EMPTY_D]
    assert len(ds) == len(small) + 2 and ds[0] < LADDER_EMPTY_D < ds[-1] < 64      # below 2^(c-1) at c = 7: the same single digit at every width
    base = dict(zip(ds, small))
    d_mid, d_huge = ds[len(small)], ds[len(small) + 1]
    if c == 7:
        return [base]
    segs = [dict(base), dict(base)]
    for j in (0, 1):
        segs[j][d_mid] = mid[j]
        if c == 11:
            segs[j][d_huge] = huge[j]
    return segs


def _ladder_scalars(counts, seed):
    vals = []
    for d, k in counts.items():
        vals += [d if i % 2 else L_ORDER - d for i in range(k)]          # equal shares (the odd one out is l - d)
    order = np.random.default_rng(seed).permutation(len(vals))
    return PC.rows([vals[i] for i in order])


@functools.lru_cache(maxsize=None)
def ladder_job(c):
    """(off, scalars, pidx, points, lens, ladder segments): the ladder segment(s), one member of MC.scalars as long as the longest of them, and one member of
    n // 2 + 1 terms -- the padded one; the first ladder segment of two is padded as well (it is the shorter one)"""
    segs = ladder_counts(c)
    ladder_lens = [sum(s.values()) for s in segs]
    n = max(ladder_lens)
    assert pick_c(n) == c, (c, n)
    lens = [ladder_lens[0], n] + ladder_lens[1:] + [n // 2 + 1]
    ladder_at = [0] + ([2] if len(segs) == 2 else [])
    off = _off(lens)
    pts = OC.points512()
    sc = MC.scalars(int(off[-1]), 80 + c).copy()
    for j, sg in enumerate(ladder_at):
        sc[int(off[sg]):int(off[sg + 1])] = _ladder_scalars(segs[j], 90 + 2 * c + j)
    return _frozen(off, sc, _pidx(int(off[-1]), 80 + c, len(pts)), pts) + (lens, ladder_at)


# ---- C1. two buckets of more than kMergeSeqParts parts in one block of the merge ------------------------------------------------------------------------
TWIN_LENS = (8200, 8200, 4200)
TWIN_SCALAR = 1 << 10                                     # c = 11: digit -2^10 in window 0 (bucket 2^10, the one k_pip_combine adds) under +1 in window 1


@functools.lru_cache(maxsize=None)
def twin_huge_job(fold=False):
    """(off, scalars, pidx, points): segment 0 all 2^10 (fold: every other one l - 2^10, the same two buckets with the other sign), segment 1 MC.scalars,
    segment 2 all 1 -- a padded member with one bucket of 66 parts"""
    off = _off(TWIN_LENS)
    pts = OC.points512()
    sc = MC.scalars(int(off[-1]), 60).copy()
    first = [neg(TWIN_SCALAR) if fold and i % 2 else TWIN_SCALAR for i in range(TWIN_LENS[0])]
    sc[:int(off[1])] = PC.rows(first)
    sc[int(off[2]):] = PC.rows([1] * TWIN_LENS[2])
    return _frozen(off, sc, _pidx(int(off[-1]), 61, len(pts)), pts)


def twin_single_job():
    """segment 0 of twin_huge_job alone: (off, scalars, pidx, points)"""
    off, sc, pidx, pts = twin_huge_job()
    n = TWIN_LENS[0]
    return off[:2].copy(), sc[:n].copy(), pidx[:n].copy(), pts


def reordered(job, order):
    """the segments of a job in another order: segment i of the result is segment order[i] of the job"""
    off, sc, pidx, pts = job
    take = np.concatenate([np.arange(int(off[s]), int(off[s + 1])) for s in order])
    lens = [int(off[s + 1]) - int(off[s]) for s in order]
    return _off(lens), np.ascontiguousarray(sc[take]), np.ascontiguousarray(pidx[take]), pts


TWIN_ORDERS = tuple(itertools.permutations(range(3)))


# ---- C2. K equal segments on both sides of the merge rule, skewed members among them -----------------------------------------------------------------
def threshold_cases(S):
    """[(c, K, terms per segment)]: K * W1 * B1 just below and just at MERGE_LANE_MIN_BUCKETS"""
    seg = {7: S + 1, 10: 4096, 11: 8200}
    out = []
    for c in WIDTHS:
        k_at = -(-merge_lane_min_buckets() // (W1(c) * B1(c)))
        out += [(c, k_at - 1, seg[c]), (c, k_at, seg[c])]
    return out


KIND_ONES, KIND_POW, KIND_TWO, KIND_RANDOM = range(4)


@functools.lru_cache(maxsize=None)
def threshold_job(c, K, seg_len):
    """(off, scalars, pidx, points, which, (off_d, sc_d, pidx_d)) in the form of OC.repeated_job over four distinct segments: every scalar 1 (one bucket
    holds the segment), every scalar 2^(c-1) (two buckets, see TWIN_SCALAR), two values at 60 % / 40 % (two buckets in every window), MC.scalars.
    Segments 0, K // 2 and K - 1 are the first three; the others take all four in turn"""
    _, _, _, pts, _, (off_d, sc_d, pidx_d) = OC.repeated_job(4, seg_len, 4, seed=50 + c)
    sc_d = sc_d.copy()
    a, b = (v % L_ORDER for v in SE.random_256(50 + c, 2))
    pick = np.random.default_rng(c).random(seg_len) < 0.6
    sc_d[KIND_ONES * seg_len:(KIND_ONES + 1) * seg_len] = PC.rows([1] * seg_len)
    sc_d[KIND_POW * seg_len:(KIND_POW + 1) * seg_len] = PC.rows([1 << (c - 1)] * seg_len)
    sc_d[KIND_TWO * seg_len:(KIND_TWO + 1) * seg_len] = PC.rows([a if p else b for p in pick])
    which = np.arange(K) % 4
    which[[0, K // 2, K - 1]] = [KIND_ONES, KIND_POW, KIND_TWO]
    sc = np.ascontiguousarray(sc_d.reshape(4, seg_len, 32)[which].reshape(-1, 32))
    pidx = np.ascontiguousarray(pidx_d.reshape(4, seg_len)[which].reshape(-1))
    off = (np.arange(K + 1, dtype=np.uint64) * seg_len).astype(np.uint32)
    return _frozen(off, sc, pidx, pts, which) + (_frozen(off_d, sc_d, pidx_d),)


# ---- D. the _dev form ----------------------------------------------------------------------------------------------------------------------------------
DEV_CHUNKS = ((257, 4096, 7), (1725, 193, 41))           # (segments, terms each = max_seg, distinct): one more than a run holds by the cap / by the grid
DEV_LONG_LENS, DEV_LONG_MAX_SEG, DEV_LONG_SEG = (300, 900, 400, 350), 400, 1


def dev_chunk_runs(n_seg, seg_len):
    """what the notes must say: the first run holds all but one segment"""
    c = pick_c(seg_len)
    return [(c, n_seg - 1, seg_len, 0), (c, 1, seg_len, n_seg - 1)]


@functools.lru_cache(maxsize=None)
def dev_chunk_job(n_seg, seg_len, distinct):
    off, sc, pidx, pts, which, d = OC.repeated_job(n_seg, seg_len, distinct, seed=n_seg)
    return _frozen(off, sc, pidx, pts, which) + (d,)


def dev_long_member_job():
    """a segment (DEV_LONG_SEG) longer than max_seg: its row is unspecified, the other rows are right"""
    return OC.job(list(DEV_LONG_LENS), seed=33)


def dev_term_path_job(S):
    return OC.job([S, 5, 0, 100, S - 1], seed=13)


def host_jobs(S):
    """[(name, off, scalars, pidx, points)] of every job above whose segments are all summed by the oracle as they stand"""
    jobs = [("catalogue%d" % c,) + catalogue_job(c)[:4] for c in WIDTHS]
    jobs += [("ladder%d" % c,) + ladder_job(c)[:4] for c in WIDTHS]
    jobs += [("twin",) + twin_huge_job(), ("twin-fold",) + twin_huge_job(True), ("twin-single",) + twin_single_job()]
    jobs += [("dev-long",) + dev_long_member_job(), ("dev-terms",) + dev_term_path_job(S)]
    return jobs


def repeated_jobs(S):
    """[(name, off, scalars, pidx, points, which, (off_d, sc_d, pidx_d))]: expected rows are OC.expected(name, off_d, sc_d, pidx_d, points)[which]"""
    jobs = [("threshold%d-%d" % (c, seg),) + threshold_job(c, K, seg) for c, K, seg in threshold_cases(S)]      # (the two K of a width share the name: the same distinct segments)
    jobs += [("chunk%d" % n,) + dev_chunk_job(n, seg, distinct) for n, seg, distinct in DEV_CHUNKS]
    return jobs
