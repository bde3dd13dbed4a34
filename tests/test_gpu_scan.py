"""Segmented prefix sums and products of scalars and running sums of points on the MI355X: zkp_sc_scan / _dev (k_sc_scan, zkp_amd/csrc/sc_scan.h),
zkp_scan_points / _dev (k_pt_scan, zkp_amd/csrc/point_scan.h) and the toolbox routing in front of them.  Scalar rows are compared with Python
integers mod l, point rows with (the sum of the known logarithms) B (tests/scan_cases.py), and both byte for byte with the host backend on the same
job.  Lengths sit around the scans' group sizes and around the smallest term counts of every launch count, all read from the library
(zkp_sc_scan_group, zkp_scan_points_group, zkp_sc_scan_launches, zkp_scan_points_launches) and never written here."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import scan_cases as SC
from zkp_amd import toolbox as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -2
BAD_STATEMENT = -10
NEVER = 2 ** 64 - 1


@pytest.fixture(scope="module")
def eng():
    from zkp_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def G(eng):
    g = int(eng._lib.zkp_sc_scan_group())
    assert g >= 8
    return g


@pytest.fixture(scope="module")
def GP(eng):
    g = int(eng._lib.zkp_scan_points_group())
    assert g >= 8
    return g


@pytest.fixture()
def always_device():
    old = [T.get_scalar_scan_min_terms(op) for op in SC.OPS], T.get_point_scan_min_terms()
    for op in SC.OPS:
        T.set_scalar_scan_min_terms(op, 0)
    T.set_point_scan_min_terms(0)
    yield
    for op, v in zip(SC.OPS, old[0]):
        T.set_scalar_scan_min_terms(op, v)
    T.set_point_scan_min_terms(old[1])


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch cannot see the GPU in this process (its HIP runtime must initialise before libzkp_mi355x.so: run with -m gpu)")
    return torch


def sc_check(eng, jb, toolbox=True, host=True):
    """Engine.scalar_scan == the integers == the host backend's bytes (== the toolbox on the device route), in both modes"""
    op, off, a, aidx = jb
    a = SC.rows(a)
    for exclusive in SC.MODES:
        got = eng.scalar_scan(op, off, a, aidx, exclusive)
        assert SC.ints(got) == SC.sc_expected(*jb, exclusive=exclusive), (op, exclusive)
        if host:
            assert (T.scalar_scan(None, op, off, a, aidx, exclusive, threads=5) == got).all()
        if toolbox:
            assert (T.scalar_scan(eng, op, off, a, aidx, exclusive) == got).all()


def pt_check(eng, jb, toolbox=True, host=True):
    off, pidx, neg = jb
    pts = SC.catalogue()
    for exclusive in SC.MODES:
        want, wst = SC.pt_expected(off, pidx, neg, exclusive)
        out, st = eng.point_scan(off, pts, pidx, neg, exclusive)
        assert (st == wst).all() and (out == want).all(), exclusive
        if host:
            h = T.point_cumsum(None, off, pts, pidx, neg, exclusive, threads=5)
            assert (h[0] == out).all() and (h[1] == st).all()
        if toolbox:
            d = T.point_cumsum(eng, off, pts, pidx, neg, exclusive)
            assert (d[0] == out).all() and (d[1] == st).all()


# ---- scalars -------------------------------------------------------------------------------------------------------------------------------------
def unit_jobs(g):
    """[pytest.param(lens, seed)] of the one-segment lengths and the shapes of tests/scan_cases.py for a group size g, one case each, its id led by
    `single` (no segment crosses a unit edge: no carry is needed) or `multi` (one does).  A scan that loses its carry fails every `multi` case and
    no `single` one."""
    named = [("one_segment_%d" % n, [n]) for n in SC.single_lengths(g)] + list(SC.shapes(g).items())
    return [pytest.param(lens, 10 + k, id=("multi-" if SC.multi_unit(lens, g) else "single-") + name) for k, (name, lens) in enumerate(named)]


def _group(name):
    from zkp_amd.engine import load_library
    return int(getattr(load_library(), name)())                  # pure arithmetic: no context, no GPU


@pytest.mark.parametrize("lens,seed", unit_jobs(_group("zkp_sc_scan_group")))
@pytest.mark.parametrize("op", SC.OPS)
def test_scalar_jobs_in_one_unit_and_over_several(eng, G, always_device, op, lens, seed):
    sc_check(eng, SC.sc_job(op, lens, seed=seed))


@pytest.mark.parametrize("op", SC.OPS)
def test_scalar_smallest_term_count_of_every_launch_count(eng, G, op):
    """one segment, and segments cut on both sides of the unit edges of every level; zkp_ctx_last_kernels names one entry per launch"""
    launches = eng._lib.zkp_sc_scan_launches
    edges = SC.launch_edges(launches)
    assert len(edges) >= 3 and edges[0][1] == 1
    eng.set_profiling(True)
    try:
        for n_launch, t in edges:
            for lens in ([t], [1, t // 2, 0, t - 1 - t // 2]):
                if sum(lens) != t or min(lens[:2]) < 1:
                    continue
                jb = SC.sc_job(op, lens, seed=t)
                sc_check(eng, jb, toolbox=False)
                eng.scalar_scan(op, jb[1], SC.rows(jb[2]))
                names = eng.last_kernels()["scalars"]
                assert launches(t) == n_launch == len(names), (t, names)
                assert all(nm.startswith("k_sc_scan<%d, " % op) for nm in names)
                up = [nm for nm in names if nm.partition("@")[0].endswith("false>")]
                down = [nm for nm in names if nm.partition("@")[0].endswith("true>")]
                assert [nm.partition("@")[2] for nm in up] == [str(k) for k in range(1, len(up) + 1)]
                assert [nm.partition("@")[2] for nm in down] == [str(k) for k in range(len(down), 0, -1)] and len(down) == len(up) + 1
        ms, total = eng.last_timing()
        assert ms["scalars"] > 0 and total >= ms["scalars"]
    finally:
        eng.set_profiling(False)


@pytest.mark.parametrize("op", SC.OPS)
def test_scalar_a_segment_over_many_units_between_short_ones(eng, G, always_device, op):
    """the long segment's ends on both sides of a unit edge of level 1 (multiples of G) and of level 2 (multiples of G * G)"""
    g2 = G * G
    for start, end in ((G - 1, g2 + 1), (G + 1, g2 - 1), (G, g2), (3, g2 + G + 1)):
        sc_check(eng, SC.sc_job(op, [2, start - 2, end - start, 1, G + 1, 4], seed=start), toolbox=False)
    sc_check(eng, SC.sc_job(op, [1] * (3 * G + 1), seed=4))                  # one row per segment


@pytest.mark.parametrize("op", SC.OPS)
def test_scalar_edge_values_as_operands(eng, G, op):
    for shift in range(0, len(SC.EDGES), 7):
        sc_check(eng, SC.sc_edge_rotation(op, G, shift), toolbox=False)
    big = SC.rows([2 ** 256 - 1] * (2 * G + 3))
    off = SC.offsets([2 * G + 3])
    want = [(k + 1) * (2 ** 256 - 1) % SC.L for k in range(2 * G + 3)] if op == SC.SUM else [pow(2 ** 256 - 1, k + 1, SC.L) for k in range(2 * G + 3)]
    assert SC.ints(eng.scalar_scan(op, off, big)) == want


def test_a_zero_factor_in_the_middle_of_a_product_scan(eng, G):
    for p in (0, 1, G - 1, G, G + 1, 2 * G + 2):
        jb = SC.sc_zero_factor(G, p)
        sc_check(eng, jb, toolbox=False)
        z, end = G + p, 3 * G + 3
        for exclusive in SC.MODES:
            got = SC.ints(eng.scalar_scan(SC.PRODUCT, jb[1], SC.rows(jb[2]), None, exclusive))
            assert all(v != 0 for v in got[:z]) and all(v != 0 for v in got[end:]) and all(v == 0 for v in got[z + 1:end])
            assert (got[z] != 0) == exclusive


@pytest.mark.parametrize("op", SC.OPS)
def test_scalar_repeated_and_skipped_indices(eng, G, always_device, op):
    for jb in SC.sc_gathers(op, G):
        sc_check(eng, jb)
    jb = SC.sc_job(op, SC.shapes(G)["ragged"], seed=5)
    a = SC.rows(jb[2])
    for exclusive in SC.MODES:
        assert (eng.scalar_scan(op, jb[1], a, None, exclusive) == eng.scalar_scan(op, jb[1], a, SC.with_arange(jb)[3], exclusive)).all()


def test_scalar_powers(eng, G, always_device):
    x = [3, 0, 1, SC.L - 1, 2 ** 256 - 1] + SC.sc_operands(SC.PRODUCT, 3, 8)
    for t in (1, 2, G + 3):
        got = T.scalar_powers(eng, SC.rows(x), t)
        assert got.shape == (len(x), t, 32)
        assert SC.ints(got) == [pow(v, i, SC.L) for v in x for i in range(t)]


# ---- points --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens,seed", unit_jobs(_group("zkp_scan_points_group")))
def test_point_jobs_in_one_unit_and_over_several(eng, GP, always_device, lens, seed):
    pt_check(eng, SC.pt_job(lens, seed=seed))


def test_point_smallest_term_count_of_every_launch_count(eng, GP):
    """one segment whose prefixes are not zero at two of three unit edges, and the same axis cut into three segments; zkp_ctx_last_kernels names
    one entry per launch: the decode, every walk, the encode"""
    launches = eng._lib.zkp_scan_points_launches
    edges = SC.launch_edges(launches)
    assert len(edges) >= 4 and edges[0][1] == 1
    eng.set_profiling(True)
    try:
        for n_launch, t in edges:
            for lens in ([t], [1, t // 2, 0, t - 1 - t // 2]):
                if sum(lens) != t or min(lens[:2]) < 1:
                    continue
                small = t <= 40 * GP * GP
                pt_check(eng, SC.pt_triples(t, lens), toolbox=False, host=small)
                kernels = eng.last_kernels()
                names = kernels["reduce"]
                assert kernels["decode"] == ["k_decode_affine"] and kernels["combine"] == ["k_pt_scan_encode"]
                assert launches(t) == n_launch == len(kernels["decode"]) + len(names) + len(kernels["combine"]), (t, kernels)
                assert sum(len(v) for v in kernels.values()) == n_launch
                assert all(nm.startswith("k_pt_scan<") for nm in names)
                up = [nm for nm in names if nm.partition("@")[0].endswith("false>")]
                down = [nm for nm in names if nm.partition("@")[0].endswith("true>")]
                assert [nm.partition("@")[2] for nm in up] == [str(k) for k in range(1, len(up) + 1)]
                assert [nm.partition("@")[2] for nm in down] == [str(k) for k in range(len(down), 0, -1)] and len(down) == len(up) + 1
        ms, total = eng.last_timing()
        assert ms["decode"] > 0 and ms["reduce"] > 0 and ms["combine"] > 0
    finally:
        eng.set_profiling(False)


def test_point_a_segment_over_many_units_between_short_ones(eng, GP):
    g2 = GP * GP
    for start, end in ((GP - 1, g2 + 1), (GP + 1, g2 - 1), (GP, g2), (3, g2 + GP + 1)):
        pt_check(eng, SC.pt_job([2, start - 2, end - start, 1, GP + 1, 4], seed=start), toolbox=False)
    pt_check(eng, SC.pt_job([1] * (3 * GP + 1), seed=4), toolbox=False)


def test_one_point_referenced_t_times_and_p_minus_p(eng, GP):
    t = 2 * GP + 5
    off = SC.offsets([t])
    out, st = eng.point_scan(off, SC.catalogue(), np.zeros(t, np.uint32))                               # B, B, B, ..: B, 2B, 3B, ..
    m = SC.multiples(range(1, t + 1))
    assert not st.any() and all((out[i] == m[i + 1]).all() for i in range(t))
    neg = (np.arange(t) % 2).astype(np.uint8)                                                           # B, -B, B, -B, ..: B, 0, B, 0, ..
    out, st = eng.point_scan(off, SC.catalogue(), np.zeros(t, np.uint32), neg)
    assert not st.any() and not out[1::2].any() and (out[0::2] == SC.catalogue()[0]).all()
    pidx = np.full(t, SC.IDENTITY_ROW, np.uint32)                                                       # identity operands
    pidx[GP] = 2
    out, st = eng.point_scan(off, SC.catalogue(), pidx)
    assert not st.any() and not out[:GP].any() and (out[GP:] == SC.catalogue()[2]).all()
    own = np.ascontiguousarray(SC.catalogue()[pidx])                                                    # pidx = None: term t is point t
    a = eng.point_scan(off, own, None, neg)
    b = eng.point_scan(off, SC.catalogue(), pidx, neg)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


def test_an_encoding_that_does_not_decode_at_the_front_middle_and_back(eng, GP):
    lens = [GP + 3, 2 * GP + 6, 5]
    off = SC.offsets(lens)
    first, last = int(off[1]), int(off[2]) - 1
    for p in (first, first + GP, last):
        jb = SC.pt_job(lens, seed=p, bad_at=(p,))
        pt_check(eng, jb, toolbox=False)
        for exclusive in SC.MODES:
            out, st = eng.point_scan(*[jb[0], SC.catalogue(), jb[1], jb[2]], exclusive)
            lo = p + 1 if exclusive else p
            assert not st[:lo].any() and st[lo:last + 1].all() and not st[last + 1:].any() and not out[lo:last + 1].any()


def test_points_against_the_host_point_sum_on_the_prefix_segments(eng, GP):
    lens = [0, 3, GP + 2, 0, 1, 7]
    off, pidx, neg = SC.pt_job(lens, seed=6, bad_at=(9,))
    pts = SC.catalogue()
    for exclusive in SC.MODES:
        p_off, p_idx, p_neg = [0], [], []
        for s in range(len(lens)):
            for t in range(int(off[s]), int(off[s + 1])):
                hi = t if exclusive else t + 1
                p_idx += list(pidx[int(off[s]):hi])
                p_neg += list(neg[int(off[s]):hi])
                p_off.append(len(p_idx))
        want, wst = T.point_sum(None, np.array(p_off, np.uint32), pts, np.array(p_idx, np.uint32), np.array(p_neg, np.uint8))
        out, st = eng.point_scan(off, pts, pidx, neg, exclusive)
        assert (st == wst).all() and (out == want).all()


# ---- the _dev forms ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", SC.OPS)
def test_scalar_dev_form_on_torch_buffers(G, op):
    """out lands in rows 1 .. T of a larger zeroed buffer and its neighbours stay zero; an index out of range leaves every row that does not depend on
    it right; the call recorded into a graph and replayed twice gives the same bytes both times"""
    torch = _torch()
    from zkp_amd.engine import Engine
    lens = SC.shapes(G)["ragged"] + [G * G + 7, 5]                           # every level a three-level plan has
    jb = SC.with_arange(SC.sc_job(op, lens, seed=6))
    _, off, a, aidx = jb
    a = SC.rows(a)
    n_seg, t = len(off) - 1, int(off[-1])
    dev = lambda x: torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to("cuda:0")      # noqa: E731
    e = Engine(0)
    stream = torch.cuda.Stream()
    e.set_stream(stream.cuda_stream)
    d_off, d_a, d_ai = dev(off), dev(a), dev(aidx)
    d_out = torch.zeros((t + 2, 32), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    try:
        for mode, exclusive in enumerate(SC.MODES):
            want = SC.sc_expected(*jb, exclusive=exclusive)
            for ai in (d_ai, None):                                          # gathered, then in order (n_a = n_terms)
                d_out.zero_()
                torch.cuda.synchronize()
                e.scalar_scan_dev(op, mode, n_seg, d_off.data_ptr(), d_a.data_ptr(), len(a), None if ai is None else ai.data_ptr(), t, d_out.data_ptr() + 32)
                e.synchronize()
                out = d_out.cpu().numpy()
                assert SC.ints(out[1:t + 1]) == want and not out[0].any() and not out[t + 1].any()
                assert (out[1:t + 1] == e.scalar_scan(op, off, a, aidx, exclusive)).all()
        # an index out of range in the long segment: every row before it and every other segment is right, nothing outside out is touched
        victim = len(lens) - 2
        wild = aidx.copy()
        p = int(off[victim]) + G + 1
        wild[p] = len(a) + 5
        d_wild = dev(wild)
        d_out.zero_()
        torch.cuda.synchronize()
        e.scalar_scan_dev(op, 0, n_seg, d_off.data_ptr(), d_a.data_ptr(), len(a), d_wild.data_ptr(), t, d_out.data_ptr() + 32)
        e.synchronize()
        out = d_out.cpu().numpy()
        got, want = SC.ints(out[1:t + 1]), SC.sc_expected(*jb, exclusive=False)
        assert got[:p] == want[:p] and got[int(off[victim + 1]):] == want[int(off[victim + 1]):]
        assert not out[0].any() and not out[t + 1].any()
        # misaligned pointers, a wrong operand length and too many terms are refused before anything is queued
        d_out.zero_()
        torch.cuda.synchronize()
        lib, h = e._lib, e._h
        O, OF, A, AI = d_out.data_ptr() + 32, d_off.data_ptr(), d_a.data_ptr(), d_ai.data_ptr()
        assert lib.zkp_sc_scan_dev(h, op, 0, n_seg, OF, A + 8, len(a), AI, t, O) == ERR_ARG
        assert lib.zkp_sc_scan_dev(h, op, 0, n_seg, OF, A, len(a), AI, t, O - 24) == ERR_ARG
        assert lib.zkp_sc_scan_dev(h, op, 0, n_seg, OF + 2, A, len(a), AI, t, O) == ERR_ARG
        assert lib.zkp_sc_scan_dev(h, op, 0, n_seg, OF, A, len(a), AI + 1, t, O) == ERR_ARG
        assert lib.zkp_sc_scan_dev(h, op, 0, n_seg, OF, A, len(a) - 1, None, t, O) == ERR_ARG
        assert lib.zkp_sc_scan_dev(h, op, 0, n_seg, OF, A, len(a), AI, 2 ** 31, O) == ERR_ARG
        assert lib.zkp_sc_scan_dev(h, op, 2, n_seg, OF, A, len(a), AI, t, O) == ERR_ARG
        assert lib.zkp_sc_scan_dev(h, 2, 0, n_seg, OF, A, len(a), AI, t, O) == ERR_ARG
        e.synchronize()
        assert not bool(d_out.any().item())
        # the graph: recorded (the same call has run above), replayed twice
        with e.capture() as cap:
            e.scalar_scan_dev(op, 1, n_seg, OF, A, len(a), AI, t, O)
        assert not bool(d_out.any().item())                                  # recorded, not run
        want = SC.sc_expected(*jb, exclusive=True)
        for _ in range(2):
            d_out.zero_()
            torch.cuda.synchronize()
            cap.graph.launch()
            e.synchronize()
            assert SC.ints(d_out.cpu().numpy()[1:t + 1]) == want
        cap.graph.close()
    finally:
        e.close()


def test_point_dev_form_on_torch_buffers(GP):
    torch = _torch()
    from zkp_amd.engine import Engine
    lens = SC.shapes(GP)["ragged"] + [GP * GP + 7, 5]
    off, pidx, neg = SC.pt_job(lens, seed=7)
    pts = SC.catalogue()
    n_seg, t = len(off) - 1, int(off[-1])
    dev = lambda x: torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to("cuda:0")      # noqa: E731
    e = Engine(0)
    stream = torch.cuda.Stream()
    e.set_stream(stream.cuda_stream)
    d_off, d_pidx, d_neg, d_pts = dev(off), dev(pidx), dev(neg), dev(pts)
    d_out = torch.zeros((t + 2, 32), dtype=torch.uint8, device="cuda:0")
    d_st = torch.zeros(t + 2, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    OF, PI, NG, P, O, ST = d_off.data_ptr(), d_pidx.data_ptr(), d_neg.data_ptr(), d_pts.data_ptr(), d_out.data_ptr() + 32, d_st.data_ptr() + 1

    def run(mode, pi=PI):
        d_out.zero_()
        d_st.zero_()
        torch.cuda.synchronize()
        e.point_scan_dev(mode, n_seg, OF, pi, NG, P, len(pts), t, O, ST)
        e.synchronize()
        out, st = d_out.cpu().numpy(), d_st.cpu().numpy()
        assert not out[0].any() and not out[t + 1].any() and not st[0] and not st[t + 1]
        return out[1:t + 1], st[1:t + 1]

    try:
        for mode, exclusive in enumerate(SC.MODES):
            want, wst = SC.pt_expected(off, pidx, neg, exclusive)
            out, st = run(mode)
            assert (out == want).all() and (st == wst).all()
            h = e.point_scan(off, pts, pidx, neg, exclusive)
            assert (h[0] == out).all() and (h[1] == st).all()
        # an index out of range flags the rows that depend on it and nothing else
        victim = len(lens) - 2
        wild = pidx.copy()
        p = int(off[victim]) + GP + 1
        wild[p] = len(pts) + 5
        d_wild = dev(wild)
        out, st = run(0, d_wild.data_ptr())
        want, wst = SC.pt_expected(off, pidx, neg, False)
        end = int(off[victim + 1])
        assert (out[:p] == want[:p]).all() and (out[end:] == want[end:]).all() and not st[:p].any() and not st[end:].any() and st[p:end].all()
        lib, h = e._lib, e._h
        d_out.zero_()
        torch.cuda.synchronize()
        assert lib.zkp_scan_points_dev(h, 0, n_seg, OF, PI, NG, P + 8, len(pts), t, O, ST) == ERR_ARG
        assert lib.zkp_scan_points_dev(h, 0, n_seg, OF, PI, NG, P, len(pts), t, O - 24, ST) == ERR_ARG
        assert lib.zkp_scan_points_dev(h, 0, n_seg, OF + 2, PI, NG, P, len(pts), t, O, ST) == ERR_ARG
        assert lib.zkp_scan_points_dev(h, 0, n_seg, OF, None, NG, P, len(pts), t, O, ST) == ERR_ARG
        assert lib.zkp_scan_points_dev(h, 0, n_seg, OF, PI, NG, P, len(pts), 2 ** 31, O, ST) == ERR_ARG
        assert lib.zkp_scan_points_dev(h, 2, n_seg, OF, PI, NG, P, len(pts), t, O, ST) == ERR_ARG
        e.synchronize()
        assert not bool(d_out.any().item())
        with e.capture() as cap:
            e.point_scan_dev(1, n_seg, OF, PI, NG, P, len(pts), t, O, ST)
        assert not bool(d_out.any().item())
        want, wst = SC.pt_expected(off, pidx, neg, True)
        for _ in range(2):
            d_out.zero_()
            d_st.zero_()
            torch.cuda.synchronize()
            cap.graph.launch()
            e.synchronize()
            assert (d_out.cpu().numpy()[1:t + 1] == want).all() and (d_st.cpu().numpy()[1:t + 1] == wst).all()
        cap.graph.close()
    finally:
        e.close()


def test_results_do_not_depend_on_what_the_workspace_held(G, GP):
    from zkp_amd.engine import Engine
    e = Engine(0, test_hooks=True)
    try:
        for word in (0xFFFFFFFF, 3):
            for op in SC.OPS:
                jb = SC.sc_job(op, [5, G * G + 3, 0, 2 * G], seed=8)         # every level of a three-level plan
                for exclusive in SC.MODES:
                    e.debug_fill_workspace(8 << 20, word)
                    assert SC.ints(e.scalar_scan(op, jb[1], SC.rows(jb[2]), None, exclusive)) == SC.sc_expected(*jb, exclusive=exclusive)
            off, pidx, neg = SC.pt_job([5, GP * GP + 3, 0, 2 * GP], seed=9, bad_at=(GP * GP,))
            for exclusive in SC.MODES:
                e.debug_fill_workspace(8 << 20, word)
                want, wst = SC.pt_expected(off, pidx, neg, exclusive)
                out, st = e.point_scan(off, SC.catalogue(), pidx, neg, exclusive)
                assert (out == want).all() and (st == wst).all()
    finally:
        e.close()


# ---- the toolbox ---------------------------------------------------------------------------------------------------------------------------------
def test_toolbox_routes_on_both_sides_of_the_thresholds(eng, G, GP):
    olds = [T.get_scalar_scan_min_terms(op) for op in SC.OPS], T.get_point_scan_min_terms()
    eng.set_profiling(True)
    try:
        for op in SC.OPS:
            thr = G + 9
            T.set_scalar_scan_min_terms(op, thr)
            for lens, device in (([3, thr - 5, 0, 1], False), ([3, thr - 5, 0, 2], True)):
                assert (sum(lens) >= thr) == device
                jb = SC.sc_job(op, lens, seed=9)
                eng.scalar_scan(SC.SUM, SC.offsets([1]), SC.rows([5]))                   # (leaves one kernel name behind)
                assert len(eng.last_kernels()["scalars"]) == 1
                got = T.scalar_scan(eng, op, jb[1], SC.rows(jb[2]))
                assert SC.ints(got) == SC.sc_expected(*jb)
                assert (len(eng.last_kernels()["scalars"]) == 3) == device               # the device route made three launches; the host route none
            T.set_scalar_scan_min_terms(op, NEVER)
            eng.scalar_scan(SC.SUM, SC.offsets([1]), SC.rows([5]))
            assert SC.ints(T.scalar_scan(eng, op, jb[1], SC.rows(jb[2]))) == SC.sc_expected(*jb) and len(eng.last_kernels()["scalars"]) == 1
        thr = GP + 9
        T.set_point_scan_min_terms(thr)
        for lens, device in (([3, thr - 5, 0, 1], False), ([3, thr - 5, 0, 2], True)):
            off, pidx, neg = SC.pt_job(lens, seed=9)
            eng.point_scan(SC.offsets([1]), SC.catalogue(), np.zeros(1, np.uint32))
            assert len(eng.last_kernels()["reduce"]) == 1
            out, st = T.point_cumsum(eng, off, SC.catalogue(), pidx, neg)
            want, wst = SC.pt_expected(off, pidx, neg)
            assert (out == want).all() and (st == wst).all()
            assert (len(eng.last_kernels()["reduce"]) == 3) == device
    finally:
        for op, v in zip(SC.OPS, olds[0]):
            T.set_scalar_scan_min_terms(op, v)
        T.set_point_scan_min_terms(olds[1])
        eng.set_profiling(False)


def test_argument_errors_write_nothing(eng, always_device):
    lib, h = eng._lib, eng._h
    _, off, a, _ = SC.sc_job(SC.SUM, [3, 0, 5], seed=4)
    a = SC.rows(a)
    idx = np.arange(8, dtype=np.uint32)
    out = np.full((8, 32), 0xEE, np.uint8)
    st = np.full(8, 0xEE, np.uint8)
    pts = np.ascontiguousarray(SC.catalogue()[:8])
    OF, A, IX, O, ST, P = (x.ctypes.data for x in (off, a, idx, out, st, pts))
    empty = np.zeros(3, np.uint32)
    for op in SC.OPS:
        for m in (0, 1):
            assert lib.zkp_sc_scan(h, op, m, 0, None, None, 0, None, None) == 0                          # n_seg = 0 and T = 0: no-ops
            assert lib.zkp_sc_scan_dev(h, op, m, 0, None, None, 0, None, 0, None) == 0
            assert lib.zkp_sc_scan(h, op, m, 2, empty.ctypes.data, None, 0, None, None) == 0
    for m in (0, 1):
        assert lib.zkp_scan_points(h, m, 0, None, None, None, None, 0, None, None) == 0
        assert lib.zkp_scan_points_dev(h, m, 0, None, None, None, None, 0, 0, None, None) == 0
        assert lib.zkp_scan_points(h, m, 2, empty.ctypes.data, None, None, None, 0, None, None) == 0
    for fn_args in ((lib.zkp_sc_scan, (h, 0, 0, 0, OF, A, 8, None, O)), (lib.zkp_sc_scan_dev, (h, 0, 0, 0, OF, A, 8, None, 8, O)),    # n_seg = 0 with operands
                    (lib.zkp_sc_scan_dev, (h, 1, 1, 0, None, A, 5, None, 0, None)), (lib.zkp_scan_points, (h, 0, 0, OF, None, None, P, 8, O, ST)),
                    (lib.zkp_scan_points_dev, (h, 0, 0, OF, None, None, P, 8, 8, O, ST)), (lib.zkp_scan_points_dev, (h, 1, 0, None, None, None, P, 5, 0, None, None))):
        assert fn_args[0](*fn_args[1]) == 0
    huge, one_idx = np.array([0, 2 ** 31], np.uint32), np.zeros(1, np.uint32)                            # more than 2^31 - 1 terms: refused before anything is read
    HG, I1 = huge.ctypes.data, one_idx.ctypes.data
    assert lib.zkp_sc_scan(h, 0, 0, 1, HG, A, 8, I1, O) == ERR_ARG
    assert lib.zkp_scan_points(h, 0, 1, HG, I1, None, P, 8, O, ST) == ERR_ARG
    assert T.lib().zkp_scalar_scan_batch(h, 0, 0, 1, HG, A, 8, I1, 0, O) == BAD_STATEMENT
    assert T.lib().zkp_point_scan_batch(h, 0, 1, HG, I1, None, P, 8, 0, O, ST) == BAD_STATEMENT
    assert lib.zkp_sc_scan(None, 0, 0, 3, OF, A, 8, None, O) == ERR_ARG                                  # a NULL context
    assert lib.zkp_sc_scan_dev(None, 0, 0, 3, OF, A, 8, None, 8, O) == ERR_ARG
    assert lib.zkp_scan_points(None, 0, 3, OF, None, None, P, 8, O, ST) == ERR_ARG
    assert lib.zkp_scan_points_dev(None, 0, 3, OF, None, None, P, 8, 8, O, ST) == ERR_ARG
    assert lib.zkp_sc_scan(None, 0, 0, 0, None, None, 0, None, None) == ERR_ARG
    for op in (2, 3, -1):                                                                               # ZKP_SC_DOT has no scan; unknown ops
        assert lib.zkp_sc_scan(h, op, 0, 3, OF, A, 8, None, O) == ERR_ARG
        assert lib.zkp_sc_scan(h, op, 0, 0, None, None, 0, None, None) == ERR_ARG
        assert lib.zkp_sc_scan_dev(h, op, 0, 3, OF, A, 8, None, 8, O) == ERR_ARG                         # (rejected before any pointer is used)
        assert T.lib().zkp_scalar_scan_batch(h, op, 0, 3, OF, A, 8, None, 0, O) == BAD_STATEMENT
    for m in (2, -1):
        assert lib.zkp_sc_scan(h, 0, m, 3, OF, A, 8, None, O) == ERR_ARG
        assert lib.zkp_sc_scan_dev(h, 0, m, 3, OF, A, 8, None, 8, O) == ERR_ARG
        assert lib.zkp_scan_points(h, m, 3, OF, None, None, P, 8, O, ST) == ERR_ARG
        assert lib.zkp_scan_points_dev(h, m, 3, OF, None, None, P, 8, 8, O, ST) == ERR_ARG
        assert T.lib().zkp_point_scan_batch(h, m, 3, OF, None, None, P, 8, 0, O, ST) == BAD_STATEMENT
    one, dec = np.array([1, 3, 3, 8], np.uint32), np.array([0, 5, 3, 8], np.uint32)
    for bad in (one, dec):
        assert lib.zkp_sc_scan(h, 0, 0, 3, bad.ctypes.data, A, 8, None, O) == ERR_ARG
        assert lib.zkp_scan_points(h, 0, 3, bad.ctypes.data, None, None, P, 8, O, ST) == ERR_ARG
        assert T.lib().zkp_scalar_scan_batch(h, 0, 0, 3, bad.ctypes.data, A, 8, None, 0, O) == BAD_STATEMENT
        assert T.lib().zkp_point_scan_batch(h, 0, 3, bad.ctypes.data, None, None, P, 8, 0, O, ST) == BAD_STATEMENT
    wild = idx.copy()
    wild[5] = 8
    assert lib.zkp_sc_scan(h, 0, 0, 3, OF, A, 8, wild.ctypes.data, O) == ERR_ARG
    assert lib.zkp_scan_points(h, 0, 3, OF, wild.ctypes.data, None, P, 8, O, ST) == ERR_ARG
    for n in (7, 9):                                                                                    # no index list: the operand must have T rows
        assert lib.zkp_sc_scan(h, 0, 0, 3, OF, A, n, None, O) == ERR_ARG
        assert lib.zkp_scan_points(h, 0, 3, OF, None, None, P, n, O, ST) == ERR_ARG
    assert lib.zkp_sc_scan(h, 0, 0, 3, None, A, 8, None, O) == ERR_ARG                                   # NULL buffers
    assert lib.zkp_sc_scan(h, 0, 0, 3, OF, None, 8, None, O) == ERR_ARG
    assert lib.zkp_sc_scan(h, 0, 0, 3, OF, A, 8, None, None) == ERR_ARG
    assert lib.zkp_sc_scan_dev(h, 0, 0, 3, None, A, 8, None, 8, O) == ERR_ARG
    assert lib.zkp_sc_scan_dev(h, 0, 0, 3, OF, A, 8, None, 8, None) == ERR_ARG
    assert lib.zkp_scan_points(h, 0, 3, None, None, None, P, 8, O, ST) == ERR_ARG
    assert lib.zkp_scan_points(h, 0, 3, OF, None, None, None, 8, O, ST) == ERR_ARG
    assert lib.zkp_scan_points(h, 0, 3, OF, None, None, P, 8, None, ST) == ERR_ARG
    assert lib.zkp_scan_points(h, 0, 3, OF, None, None, P, 8, O, None) == ERR_ARG
    assert lib.zkp_scan_points_dev(h, 0, 3, OF, None, None, P, 8, 8, O, None) == ERR_ARG
    assert (out == 0xEE).all() and (st == 0xEE).all()


@pytest.mark.parametrize("name,args,needle", [("feldman_vss_batch.py", ["64", "5", "9"], "576 of 576 shares verified"),
                                              ("running_tally_batch.py", ["16", "40"], "640 of 640 running totals decrypted")])
def test_the_examples_on_the_engine(name, args, needle):
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "examples", name)] + args, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert needle in r.stdout, r.stdout
