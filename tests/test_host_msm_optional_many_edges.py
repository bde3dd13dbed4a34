"""The jobs of tests/msm_optional_many_edge_cases.py on the host backend (no GPU), and what each construction puts into which bucket.

Every job runs through toolbox.optional_multiscalar_mul(None, ...) at 1 and 5 threads, byte for byte and status for status against the oracle's
msm_many -- the expectations tests/test_gpu_msm_optional_many_edges.py holds the bucket kernels to.  The host has no bucket method, so what the
jobs are FOR is asserted on the scalars themselves with SE.pip_digits, the Python restatement of the device's digit code: the ladder's bucket sizes
and the part counts they give, the two huge buckets of the twin job and the merge blocks they fall into, the slots of the catalogue values, K on
both sides of the merge rule."""
import os
import re

import numpy as np
import pytest

from tests import msm_optional_many_cases as OC
from tests import msm_optional_many_edge_cases as EC
from tests import scalar_edge_cases as SE
from zkp_amd import toolbox as T

THREADS = (1, 5)


@pytest.fixture(scope="module")
def S():
    from zkp_amd.engine import load_library
    return int(load_library().zkp_msm_optional_many_min_segment())          # pure arithmetic: no context, no GPU


def _int(row):
    return int.from_bytes(bytes(row), "little")


def bucket_counts(sc, c):
    """{(window, bucket index): [entries, entries with a negative sign]} of the scalars of one segment at width c, the carry window included"""
    rows, counts = np.unique(np.ascontiguousarray(sc), axis=0, return_counts=True)
    out = {}
    for row, k in zip(rows, counts):
        digits, carry, fold = SE.pip_digits(_int(row), c)
        for w, d in enumerate(digits + [carry]):
            if d:
                e = out.setdefault((w, abs(d)), [0, 0])
                e[0] += int(k)
                e[1] += int(k) * int((d < 0) != bool(fold))
    return out


def test_the_constants_come_from_the_sources():
    L, big = EC.part_L(), EC.merge_seq_parts()
    assert L >= 4 and big >= 64 and EC.merge_lane_min_buckets() >= 1 << 16
    # part_len() restates the device function: clamp(ceil(sqrt(cnt)), L, 4 L)
    assert re.search(r"const uint32_t r = \(uint32_t\)ceilf\(sqrtf\(\(float\)cnt\)\);\s*return r > 4 \* L \? 4 \* L : \(r > L \? r : L\);", EC._kernels())
    edges = EC.count_edges()
    assert edges == sorted(set(edges)) and len(edges) == 11
    parts = [EC.part_count(n) for n in edges]
    assert parts[:4] == [1, 2, 2, 3]
    assert EC.part_len(edges[3]) == L and EC.part_len(edges[4]) == L + 1 and EC.part_len(edges[5]) == L + 1 and EC.part_len(edges[6]) == L + 2
    assert parts[4] == parts[3 + 1] and parts[5] == L + 1 and parts[6] == L + 1
    assert EC.part_len(edges[7]) == EC.part_len(edges[8]) == 4 * L and parts[7:9] == [4 * L, 4 * L + 1]
    assert parts[9:] == [big, big + 1]                                    # the last bucket the quads sum in sequence, the first the whole block sums
    for c in EC.WIDTHS:
        assert EC.pick_c(EC.LONGEST[c]) == c
    assert re.search(r"if \(n < \(1u << 12\)\) return 7;\s*if \(n < \(1u << 13\)\) return 10;\s*if \(n < \(1u << 21\)\) return 11;", EC._kernels())


@pytest.mark.parametrize("c", EC.WIDTHS)
def test_catalogue_values_sit_in_the_named_slots_of_two_segments(c):
    off, sc, pidx, pts, placed = EC.catalogue_job(c)
    lens = EC.catalogue_lens(c)
    n = max(lens)
    assert len(lens) == 6 and n == EC.LONGEST[c] and n // 2 + 1 in lens and all(2 * x > n for x in lens)
    vals = EC.catalogue_values(c)
    assert len(vals) == len(set(vals)) and all(0 <= v < 2 ** 256 for v in vals)
    named = [v for name, v in SE.CATALOGUE if "pip%d:" % c in name]
    assert len(named) >= 10 and set(named) <= set(vals)
    assert {0, 1, OC.L - 1, OC.L, OC.L + 1, 2 ** 256 - 1, SE.HALF, SE.HALF + 1} <= set(vals)
    assert all(v in placed and EC.neg(v) in placed for v in EC.catalogue_base(c))
    for v in vals:
        where = placed[v]
        assert len({sg for sg, _ in where}) >= 2, hex(v)
        for sg, slot in where:
            assert slot < lens[sg] and _int(sc[int(off[sg]) + slot]) == v
    used = {(sg, slot) for where in placed.values() for sg, slot in where}
    assert len(used) == sum(len(w) for w in placed.values())            # no slot twice
    for sg, m in enumerate(lens):
        for slot in (0, 255, 256, m - 1):
            assert slot >= m or (sg, slot) in used, (sg, slot)
    short = lens.index(n // 2 + 1)
    assert (short, n // 2) in used                                        # the slot next to the padding
    # a value of the recoder's own list reaches it unfolded or folded as the catalogue says, and the digits recombine to it
    for v in named:
        digits, carry, fold = SE.pip_digits(v, c)
        assert SE.recombine(digits, carry, c) == (OC.L - v if fold else v)


@pytest.mark.parametrize("c", EC.WIDTHS)
def test_ladder_buckets_hold_exactly_the_counts(c):
    off, sc, pidx, pts, lens, ladder_at = EC.ladder_job(c)
    n = max(lens)
    edges = EC.count_edges()
    assert EC.pick_c(n) == c and all(2 * x > n for x in lens) and lens[-1] == n // 2 + 1 and lens[1] == n
    seen = []
    for sg, want in zip(ladder_at, EC.ladder_counts(c)):
        for d in want:                                                    # each d alone in window 0, l - d folded onto it
            assert SE.pip_digits(d, c) == ([d] + [0] * (SE.pip_windows(c) - 1), 0, 0)
            assert SE.pip_digits(OC.L - d, c) == ([d] + [0] * (SE.pip_windows(c) - 1), 0, 1)
        got = bucket_counts(sc[int(off[sg]):int(off[sg + 1])], c)
        assert {k: v[0] for k, v in got.items()} == {(0, d): k for d, k in want.items()}          # nothing in a higher window
        assert all(v[1] == (v[0] + 1) // 2 for v in got.values())         # equal shares of both signs
        assert EC.LADDER_EMPTY_D not in want and min(want) < EC.LADDER_EMPTY_D < max(want)
        seen += list(want.values())
    holds = [k for k in edges if k < {7: 4096, 10: 8192, 11: 1 << 21}[c] - sum(edges[:7])]
    assert sorted(set(seen)) == holds, (seen, holds)
    assert len(holds) == {7: 7, 10: 9, 11: 11}[c]
    if len(ladder_at) == 2:
        a, b = (EC.ladder_counts(c)[j] for j in (0, 1))
        assert all(a[d] == b[d] or a[d] + 1 == b[d] for d in a)           # the two sides of an edge lie in two different segments
    # the random member has terms in every window up to the top one of a canonical scalar
    rnd = bucket_counts(sc[int(off[1]):int(off[2])][:300], c)
    assert {w for w, _ in rnd} >= set(range(252 // c))


def test_twin_job_has_two_huge_buckets_in_one_merge_block():
    c, big = 11, EC.merge_seq_parts()
    for fold in (False, True):
        off, sc, pidx, pts = EC.twin_huge_job(fold)
        assert np.diff(off.astype(np.int64)).tolist() == list(EC.TWIN_LENS) and EC.pick_c(max(EC.TWIN_LENS)) == c
        got = bucket_counts(sc[:int(off[1])], c)
        n0 = EC.TWIN_LENS[0]
        assert {k: v[0] for k, v in got.items()} == {(0, 1 << 10): n0, (1, 1): n0}      # exactly two non-empty buckets
        assert got[(0, 1 << 10)][1] == (n0 if not fold else n0 // 2) and got[(1, 1)][1] == (0 if not fold else n0 // 2)
        assert all(EC.part_count(v[0]) > big for v in got.values()) and EC.part_len(n0) == 4 * EC.part_L()
        assert EC.part_count(n0 - 9) <= big                               # (8,192 entries would not do)
        ones = bucket_counts(sc[int(off[2]):], c)
        assert {k: v[0] for k, v in ones.items()} == {(0, 1): EC.TWIN_LENS[2]} and EC.part_count(EC.TWIN_LENS[2]) == 66
    assert all(2 * x > max(EC.TWIN_LENS) for x in EC.TWIN_LENS)          # one class whatever the order
    # flat bucket indices (b W1 + w) B1 + bucket for every place b the segment can take in the run: one block of the quad form (64 buckets) and one of
    # the lane form (256)
    for b in range(3):
        flat = [(b * EC.W1(c) + w) * EC.B1(c) + d for w, d in ((0, 1 << 10), (1, 1))]
        assert flat[0] // 64 == flat[1] // 64 and flat[0] // 256 == flat[1] // 256, (b, flat)
    assert [(0 * EC.W1(c) + w) * EC.B1(c) + d for w, d in ((0, 1 << 10), (1, 1))] == [1024, 1026]
    off1, sc1, _, _ = EC.twin_single_job()
    assert off1.tolist() == [0, EC.TWIN_LENS[0]] and {_int(r) for r in sc1} == {EC.TWIN_SCALAR}
    # every order of the three segments is the same three segments
    job = EC.twin_huge_job()
    for order in EC.TWIN_ORDERS:
        o_off, o_sc, o_pidx, _ = EC.reordered(job, order)
        for i, s in enumerate(order):
            assert (o_sc[int(o_off[i]):int(o_off[i + 1])] == job[1][int(job[0][s]):int(job[0][s + 1])]).all()
            assert (o_pidx[int(o_off[i]):int(o_off[i + 1])] == job[2][int(job[0][s]):int(job[0][s + 1])]).all()


def test_threshold_jobs_straddle_the_merge_rule(S):
    cases = EC.threshold_cases(S)
    assert [(c, K) for c, K, _ in cases] == [(7, 212), (7, 213), (10, 37), (10, 38), (11, 20), (11, 21)]
    assert [EC.W1(c) * EC.B1(c) for c in EC.WIDTHS] == [2470, 13851, 25625]
    for c, K, seg in cases:
        nb = K * EC.W1(c) * EC.B1(c)
        assert (nb >= EC.merge_lane_min_buckets()) == (K in (213, 38, 21)) and EC.pick_c(seg) == c and seg > S
        off, sc, pidx, pts, which, (off_d, sc_d, pidx_d) = EC.threshold_job(c, K, seg)
        assert len(off) == K + 1 and which[[0, K // 2, K - 1]].tolist() == [EC.KIND_ONES, EC.KIND_POW, EC.KIND_TWO]
        assert set(which.tolist()) == {0, 1, 2, 3} and (sc.reshape(K, seg, 32) == sc_d.reshape(4, seg, 32)[which]).all()
        kinds = [bucket_counts(sc_d[k * seg:(k + 1) * seg], c) for k in range(3)]
        assert {k: v[0] for k, v in kinds[0].items()} == {(0, 1): seg}
        assert {k: v[0] for k, v in kinds[1].items()} == {(0, 1 << (c - 1)): seg, (1, 1): seg}
        per_window = {}
        for (w, _), v in kinds[2].items():
            per_window.setdefault(w, []).append(v[0])
        assert len(per_window) >= 252 // c and all(len(v) <= 2 and sum(v) <= seg for v in per_window.values())      # (less than seg where a digit is 0)
        assert any(len(v) == 2 and 0.5 * seg < max(v) < 0.7 * seg for v in per_window.values())


def check(name, off, sc, pidx, points):
    want, want_st = OC.expected(name, off, sc, pidx, points)
    for t in THREADS:
        got, st = T.optional_multiscalar_mul(None, off, sc, points, pidx, threads=t)
        assert (st == want_st).all(), (name, t)
        assert (got == want).all(), (name, t)
    return want, want_st


N_HOST_JOBS, N_REPEATED_JOBS = 11, 8


@pytest.mark.parametrize("which", range(N_HOST_JOBS))
def test_every_job_on_the_host_route(S, which):
    jobs = EC.host_jobs(S)
    assert len(jobs) == N_HOST_JOBS and len({j[0] for j in jobs}) == N_HOST_JOBS
    name, off, sc, pidx, pts = jobs[which]
    want, st = check(name, off, sc, pidx, pts)
    assert not st.any()
    empty = np.diff(off.astype(np.int64)) == 0
    assert want[~empty].any(axis=1).all() and not want[empty].any(), name


def test_the_twin_jobs_are_three_different_questions():
    """the fold variant is another sum, not the same one twice; the single segment is segment 0 of the job"""
    assert (OC.expected("twin", *EC.twin_huge_job())[0][0] != OC.expected("twin-fold", *EC.twin_huge_job(True))[0][0]).any()
    assert (OC.expected("twin", *EC.twin_huge_job())[0][0] == OC.expected("twin-single", *EC.twin_single_job())[0][0]).all()


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("job", range(N_REPEATED_JOBS))
def test_every_repeated_job_on_the_host_route(S, job, threads):
    """the host route sums every segment of the job, the oracle the distinct ones: up to 2^20 terms, one case per thread count"""
    jobs = EC.repeated_jobs(S)
    assert len(jobs) == N_REPEATED_JOBS
    name, off, sc, pidx, pts, which, (off_d, sc_d, pidx_d) = jobs[job]
    want_d, st_d = OC.expected(name, off_d, sc_d, pidx_d, pts)
    assert not st_d.any() and len({bytes(r) for r in want_d}) == len(want_d), name
    got, st = T.optional_multiscalar_mul(None, off, sc, pts, pidx, threads=threads)
    assert not st.any() and (got == want_d[which]).all(), name


def test_the_dev_jobs_sit_at_the_limits_they_are_for(S):
    for n_seg, seg, _ in EC.DEV_CHUNKS:
        assert EC.dev_chunk_runs(n_seg, seg)[0][1] == n_seg - 1
    n_seg, seg, _ = EC.DEV_CHUNKS[1]
    assert n_seg - 1 == 65535 // EC.W1(7) and seg == S + 1               # the grid cuts: K * W1 <= 65535
    n_seg, seg, _ = EC.DEV_CHUNKS[0]
    src = open(os.path.join(EC.ROOT, "zkp_amd", "csrc", "pip_segments.h")).read()
    cap = 1 << int(re.search(r"constexpr uint64_t kPipRunCapTerms = 1u << (\d+);", src).group(1))
    assert (n_seg - 1) * seg == cap                                        # the cap cuts
    lens = list(EC.DEV_LONG_LENS)
    assert lens[EC.DEV_LONG_SEG] > EC.DEV_LONG_MAX_SEG == max(x for i, x in enumerate(lens) if i != EC.DEV_LONG_SEG)
